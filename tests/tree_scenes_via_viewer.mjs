// tests/tree_scenes_via_viewer.mjs — the octree cull of a dynamicMode mesh through the JS drop-in (node/SplatMesh.mjs): a mesh of
// several scenes is built with finalBuild, so that buildSplatTree makes one sub-tree per scene; then, per camera pose,
//   walk<k>.u32     the list of the Viewer's own gatherSceneNodesForSort text (cut from the reference into
//                   <bundle>/viewer_cut.json, as tests/gpu_sort_via_viewer.mjs uses it) walking HipSplatTree.subTrees with the
//                   mesh's getSceneTransform - only where the bundle exists (`-` = no bundle)
//   device<k>.u32   the list of HipSplatTree.gather, the device-side gather (gs_tree_gather_scenes)
//   frame_<name>.u8 with `draw`: the frame of every named draw order through updateRenderIndexes / updateUniforms / renderFrame, the
//                   mesh's matrixWorld set to identity first (the cull of a dynamic mesh leaves it out, the draw does not)
// and meta.json: {subTrees: leaves per sub-tree, visited, counted, walk: [splatRenderCount] | null, device: [splatRenderCount]}.
// The splat buffers are stand-ins with the methods the drop-in calls on a reference SplatBuffer; every scene's transform is the
// case's matrix, set exactly (the scenes' updateTransform is replaced: composing it from a quaternion would round differently).
// usage: node --experimental-loader ../oracle/three_loader.mjs tree_scenes_via_viewer.mjs <bundle|-> <in.json> <outDir>
//   in.json: {scenes: [[x, y, z, ...]], transforms: [[16]], meshWorld: [16], poses: [{matrixWorld, fov, width, height, gatherAll}],
//             draw: {width, height, focal: [fx, fy], matrixWorld, view, proj, orders: {name: [global indexes, far to near]}} | absent}
import fs from 'fs';
import path from 'path';
import { pathToFileURL } from 'url';
import * as THREE from 'three';
import { SplatMesh } from '../node/SplatMesh.mjs';
const [bundleDir, inPath, outDir] = process.argv.slice(2);
const a = JSON.parse(fs.readFileSync(inPath, 'utf8'));

class StandInBuffer {
  constructor(centers) {
    Object.assign(this, { centers, splatCount: centers.length / 3, compressionLevel: 0, sceneCenter: new THREE.Vector3(),
                          minSphericalHarmonicsCoeff: -1.5, maxSphericalHarmonicsCoeff: 1.5 });
  }
  getSplatCount() { return this.splatCount; }
  getMaxSplatCount() { return this.splatCount; }
  getMinSphericalHarmonicsDegree() { return 0; }
  fillSplatCenterArray(out, transform, from = 0, to = this.splatCount - 1, dest = 0) {
    const v = new THREE.Vector3();
    for (let i = from; i <= to; i++) {
      v.set(this.centers[3 * i], this.centers[3 * i + 1], this.centers[3 * i + 2]);
      if (transform) v.applyMatrix4(transform);
      out[(i - from + dest) * 3] = v.x; out[(i - from + dest) * 3 + 1] = v.y; out[(i - from + dest) * 3 + 2] = v.z;
    }
  }
  fillSplatCovarianceArray(out, transform, from = 0, to = this.splatCount - 1, dest = 0) {
    for (let i = from; i <= to; i++) { const o = (i - from + dest) * 6; out[o] = out[o + 3] = out[o + 5] = 0.0025; out[o + 1] = out[o + 2] = out[o + 4] = 0; }
  }
  fillSplatColorArray(out, minimumAlpha, from = 0, to = this.splatCount - 1, dest = 0) {
    for (let i = from; i <= to; i++) { const o = (i - from + dest) * 4; out[o] = 200; out[o + 1] = 120; out[o + 2] = 60; out[o + 3] = 255; }
  }
}

const run = async () => {
  const mesh = new SplatMesh(0, true, false, false, 1, false, true, false, 1024, 0, 0, 1.0, 0.3);      // dynamicMode
  const buffers = a.scenes.map((c) => new StandInBuffer(c));
  const treeReady = new Promise((resolve) => mesh.onSplatTreeReady(resolve));
  mesh.build(buffers, buffers.map(() => ({})), true, true);
  await treeReady;
  mesh.scenes.forEach((sc, s) => { sc.updateTransform = function() { this.transform.fromArray(a.transforms[s]); }; sc.updateTransform(); });
  mesh.matrixWorld.fromArray(a.meshWorld);
  const tree = mesh.getSplatTree(), n = mesh.getSplatCount();

  let gather = null;
  if (bundleDir !== '-') {
    const { Constants } = await import(pathToFileURL(path.join(bundleDir, 'src/Constants.js')).href);
    const text = JSON.parse(fs.readFileSync(path.join(bundleDir, 'viewer_cut.json'), 'utf8')).gatherSceneNodesForSort;
    gather = new Function('THREE', 'Constants', 'return (' + text.slice(text.indexOf('function')) + ')();')(THREE, Constants);
  }
  let visited = 0;
  tree.visitLeaves(() => visited++);
  const meta = { subTrees: tree.subTrees.map((t) => t.nodesWithIndexes.length), visited, counted: tree.countLeaves(), walk: gather ? [] : null, device: [] };
  a.poses.forEach((p, k) => {
    const camera = { fov: p.fov, matrixWorld: new THREE.Matrix4().fromArray(p.matrixWorld) };
    if (gather) {
      const viewer = { getRenderDimensions(v) { v.x = p.width; v.y = p.height; }, camera, splatMesh: mesh, sortWorkerIndexesToSort: new Uint32Array(n) };
      const r = gather.call(viewer, !!p.gatherAll);
      meta.walk.push(r.splatRenderCount);
      fs.writeFileSync(path.join(outDir, `walk${k}.u32`), Buffer.from(viewer.sortWorkerIndexesToSort.buffer, 0, 4 * r.splatRenderCount));
    }
    const out = new Uint32Array(tree.splats);
    const r = tree.gather(camera, { x: p.width, y: p.height }, !!p.gatherAll, null, out);
    meta.device.push(r.splatRenderCount);
    fs.writeFileSync(path.join(outDir, `device${k}.u32`), Buffer.from(out.buffer, 0, 4 * r.splatRenderCount));
  });
  if (a.draw) {
    const d = a.draw, camera = { matrixWorld: new THREE.Matrix4().fromArray(d.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(d.proj),
                                 matrixWorldInverse: new THREE.Matrix4().fromArray(d.view) };
    mesh.matrixWorld.identity();
    for (const name of Object.keys(d.orders)) {
      mesh.updateRenderIndexes(Uint32Array.from(d.orders[name]), d.orders[name].length);
      mesh.updateUniforms({ x: d.width, y: d.height }, d.focal[0], d.focal[1], false, 1.0, 1.0);
      fs.writeFileSync(path.join(outDir, `frame_${name}.u8`), Buffer.from(mesh.renderFrame(camera).data));
    }
  }
  fs.writeFileSync(path.join(outDir, 'meta.json'), JSON.stringify(meta));
  await mesh.dispose();
  console.log(JSON.stringify({ ok: true, subTrees: meta.subTrees }));
};
run().catch((e) => { console.error(e); process.exit(1); });
