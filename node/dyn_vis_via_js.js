// One visibility-culled frame of a DYNAMIC mesh and a dynamic-mode sort worker through the JS shim (test driver):
// setVisibilityCull(true) -> project -> {sort: {.., transforms}} -> draw.  usage: node dyn_vis_via_js.js <in.bin> <expect.bin> <out.bin>
// in.bin: uint32 header {n, width, height, sceneCount, 0, 0, 0, 0}, then centers F32[3n], cov F32[6n], rgba U8[4n], meshScene U32[n],
// sorterScene U32[n], intCenters I32[4n], modelView F32[16], proj F32[16], view F32[16], camPos F32[3], focal F32[2], sortMvp F32[16],
// transforms F32[16 * sceneCount], invCamPos F32[4 * sceneCount], visible U32[sceneCount]
// expect.bin: the frame U8[4 * width * height] and the sorted list U32[kept] another binding recorded for the same input
// out.bin: this run's frame and list, laid out the same; stdout: one JSON line {kept, listEqual, frameEqual}
'use strict';
const fs = require('fs');
const gs = require('./gsplat.js');
const [inPath, expectPath, outPath] = process.argv.slice(2);
const buf = fs.readFileSync(inPath);
const ab = buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength);
const [n, width, height, sceneCount] = new Uint32Array(ab, 0, 8);
let off = 32;
const take = (Type, count) => { const a = new Type(ab.slice(off, off + count * Type.BYTES_PER_ELEMENT)); off += count * Type.BYTES_PER_ELEMENT; return a; };
const centers = take(Float32Array, 3 * n), cov = take(Float32Array, 6 * n), rgba = take(Uint8Array, 4 * n);
const meshScene = take(Uint32Array, n), sorterScene = take(Uint32Array, n), intCenters = take(Int32Array, 4 * n);
const modelView = take(Float32Array, 16), proj = take(Float32Array, 16), view = take(Float32Array, 16), camPos = take(Float32Array, 3);
const focal = take(Float32Array, 2), sortMvp = take(Float32Array, 16);
const transforms = take(Float32Array, 16 * sceneCount), invCamPos = take(Float32Array, 4 * sceneCount), visible = take(Uint32Array, sceneCount);

const mesh = new gs.SplatMeshHIP(n, { sphericalHarmonicsDegree: 0, dynamicMode: true, enableOptionalEffects: true });
mesh.build(centers, cov, rgba, null);
mesh.setSceneIndexes(meshScene);
mesh.setScenes({ sceneCount, transforms, invCamPos, opacity: new Float32Array(sceneCount).fill(1), visible });
mesh.updateUniforms({ x: width, y: height }, focal[0], focal[1], false, 1.0, 1.0);
mesh.setCameraMatrices(modelView, proj, camPos, view);

const worker = gs.createSortWorker(n, false, false, true, true);          // integer centres, dynamic mode
worker.synchronous = true;
worker.onmessage = (e) => {
  if (!e.data.sortDone) return;
  const list = e.data.sortedIndexes;
  mesh.useSortWorkerResult(worker, n);
  const { pixels } = mesh.render();
  const frame = Buffer.from(pixels.buffer, pixels.byteOffset, pixels.byteLength);
  const got = Buffer.concat([frame, Buffer.from(list.buffer, list.byteOffset, list.byteLength)]);
  const expect = fs.readFileSync(expectPath);
  fs.writeFileSync(outPath, got);
  console.log(JSON.stringify({ kept: e.data.splatRenderCount, listEqual: Buffer.compare(got.subarray(frame.length), expect.subarray(frame.length)) === 0,
                               frameEqual: Buffer.compare(frame, expect.subarray(0, frame.length)) === 0 }));
  worker.terminate();
  mesh.dispose();
};
worker.postMessage({ centers: intCenters.buffer, sceneIndexes: sorterScene.buffer, range: { from: 0, to: n - 1, count: n } });
mesh.useSortWorkerResult(worker, n);
worker.bindMesh(mesh);
worker.setVisibilityCull(true);
mesh.project();
worker.postMessage({ sort: { modelViewProj: Array.from(sortMvp), splatRenderCount: n, splatSortCount: n, usePrecomputedDistances: false,
                             transforms: Array.from(transforms) } });
