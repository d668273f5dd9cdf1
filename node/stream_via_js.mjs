// Test driver: a file streamed into the drop-in (node/SplatMesh.mjs buildFromStream) piece by piece.
// usage: node stream_via_js.mjs <in.json> <outDir>
// in.json: {file, format (AssetFormat), shDegree, ends: [byte offset at which every append ends, the last one the file's size],
//           modelViewProj (the sort's), width, height, focal, matrixWorld, view, proj}
// Three meshes over the same file: `pieces` receives it in ends.length appends, `folded` the same with foldRunsAtFinalBuild = true,
// `whole` in one append.  Every append is an update build: the rows it made ready go to the mesh and to the sort worker on the
// device.  Of each: the sort worker's order -> <outDir>/<name>.order.u32, the storage position of every splat (the addon's test
// hook meshStoragePositions) -> <name>.pos.u32, the frame drawn with that order -> <name>.u8; and on stdout what every append
// reported.
import fs from 'fs';
import path from 'path';
import { createRequire } from 'module';
import * as THREE from 'three';
import { SplatMesh } from './SplatMesh.mjs';
const gs = createRequire(import.meta.url)('./gsplat.js');
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8')), outDir = process.argv[3];
const bytes = new Uint8Array(fs.readFileSync(a.file));

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);

const load = async (name, ends, fold) => {
  const mesh = new SplatMesh(0, false, false, false, 1, false, true, false, 1024, 0, a.shDegree, 1.0, 0.3);
  if (fold) mesh.foldRunsAtFinalBuild = true;
  const stream = gs.assetStreamOpen(a.format, a.shDegree, bytes.length);
  let worker = null;
  const sorter = {                                         // the worker is sized from the header, which the first appends may not hold
    uploadAssetCenters: (...args) => {
      if (!worker) { worker = gs.createSortWorker(stream.info.splatCount, false, true, true, false); worker.synchronous = true; }
      return worker.uploadAssetCenters(...args);
    },
  };
  const appends = [];
  let at = 0;
  ends.forEach((end, k) => {
    const update = mesh.buildFromStream(stream, bytes.subarray(at, end), k === ends.length - 1, sorter);
    appends.push({ bytes: end, ready: stream.info.splatsReady, from: update ? update.from : null, count: update ? update.count : null });
    at = end;
  });
  const n = stream.info.splatCount;
  const order = await new Promise((resolve) => {
    worker.onmessage = (e) => { if (e.data.sortDone) resolve(e.data.sortedIndexes); };
    worker.postMessage({ sort: { modelViewProj: Float32Array.from(a.modelViewProj), splatRenderCount: n, splatSortCount: n } });
  });
  fs.writeFileSync(path.join(outDir, `${name}.order.u32`), Buffer.from(order.buffer, order.byteOffset, order.byteLength));
  const pos = new Uint32Array(n);
  gs.addon.meshStoragePositions(mesh.core.handle, pos);
  fs.writeFileSync(path.join(outDir, `${name}.pos.u32`), Buffer.from(pos.buffer));
  mesh.updateRenderIndexes(order, n);
  mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
  fs.writeFileSync(path.join(outDir, `${name}.u8`), Buffer.from(mesh.renderFrame(camera).data));
  const result = { splatCount: n, complete: stream.info.complete, uploaded: mesh.core.getSplatCount(), treeLeaves: mesh.getSplatTree() ? mesh.getSplatTree().countLeaves() : null, appends };
  worker.terminate();
  await mesh.dispose();
  gs.assetStreamClose(stream);
  return result;
};

(async () => {
  const out = {};
  for (const [name, ends, fold] of [['pieces', a.ends, false], ['folded', a.ends, true], ['whole', [bytes.length], false]]) out[name] = await load(name, ends, fold);
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
