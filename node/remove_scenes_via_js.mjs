// Test driver: SplatMesh.removeScenes of the drop-in (node/SplatMesh.mjs) on a three-scene mesh, against a drop-in mesh built from
// the two remaining buffers.  usage: node remove_scenes_via_js.mjs <in.json>
// in.json: {scenes: [{centers, cov, rgba (plain arrays), position}], dynamic, order (the draw order of a dynamic run), width, height,
//           focal, matrixWorld, view, proj, sortMvp}
// Static run: both meshes feed a sort worker with getIntegerCenters; the edited one's worker receives `sort`, `remove`, `sort`
// back to back, so the removal waits in the worker's queue behind the asynchronous sort in flight.  The lists handed to
// updateRenderIndexes and the frames must be equal, and so the host bookkeeping and the region's averaged centre (its radii only
// ever grow: the edited mesh's must cover the fresh one's).  Dynamic run: the scenes'
// transforms are uniforms; the frames from one shared order must be equal.  Then the fall-back: a mesh with a buffer that is
// still loading cannot be edited on the device and is built afresh - same frame again.  stdout: one JSON line.
import fs from 'fs';
import { createRequire } from 'module';
import * as THREE from 'three';
import { SplatMesh } from './SplatMesh.mjs';
const require = createRequire(import.meta.url);
const gs = require('./gsplat.js');
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

class StandInBuffer {                                       // the methods the drop-in calls on a reference SplatBuffer
  constructor(scene) {
    this.s = scene;
    this.max = scene.centers.length / 3;
    Object.assign(this, { splatCount: this.max, compressionLevel: 0, sceneCenter: new THREE.Vector3(0, 0, 0),
                          minSphericalHarmonicsCoeff: -1.5, maxSphericalHarmonicsCoeff: 1.5 });
  }
  getSplatCount() { return this.splatCount; }
  getMaxSplatCount() { return this.max; }
  getMinSphericalHarmonicsDegree() { return 0; }
  _copy(src, width, out, from = 0, to = this.splatCount - 1, dest = 0) {
    for (let i = from; i <= to; i++) for (let k = 0; k < width; k++) out[(i - from + dest) * width + k] = src[i * width + k];
  }
  fillSplatCenterArray(out, transform, from = 0, to = this.splatCount - 1, dest = 0) {
    const v = new THREE.Vector3();
    for (let i = from; i <= to; i++) {
      v.set(this.s.centers[3 * i], this.s.centers[3 * i + 1], this.s.centers[3 * i + 2]);
      if (transform) v.applyMatrix4(transform);
      out[(i - from + dest) * 3] = v.x; out[(i - from + dest) * 3 + 1] = v.y; out[(i - from + dest) * 3 + 2] = v.z;
    }
  }
  fillSplatCovarianceArray(out, transform, from, to, dest) { this._copy(this.s.cov, 6, out, from, to, dest); }
  fillSplatColorArray(out, minimumAlpha, from, to, dest) { this._copy(this.s.rgba, 4, out, from, to, dest); }
}

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);
const buffers = a.scenes.map((s) => new StandInBuffer(s)), options = a.scenes.map((s) => ({ position: s.position }));
const meshOf = (which) => {
  const mesh = new SplatMesh(0, !!a.dynamic, false, false, 1, false, true, false, 1024, 0, 0, 1.0, 0.3);
  mesh.build(which.map((k) => buffers[k]), which.map((k) => options[k]), true, false);
  return mesh;
};
const frameOf = (mesh, order, count) => {
  mesh.updateRenderIndexes(order, count);
  mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
  return Buffer.from(mesh.renderFrame(camera).data);
};
const stateOf = (m) => JSON.stringify([m.getSplatCount(), m.getSplatCount(true), m.getMaxSplatCount(), m.getSceneCount(), m.lastBuildSplatCount,
  m.lastBuildMaxSplatCount, m.lastBuildSceneCount, m.lastBuildScenes.map((sc) => buffers.indexOf(sc.splatBuffer)), m.sceneOptions,
  m.globalSplatIndexToLocalSplatIndexMap, m.globalSplatIndexToSceneIndexMap, m.scenes.map((sc) => Array.from(sc.transform.elements)),
  m.calculatedSceneCenter.toArray(), m.visible]);     // (the region's radii only ever grow: they keep what the three scenes reached)
const total = buffers.reduce((n, b) => n + b.max, 0), left = buffers[0].max + buffers[2].max;

// every sortDone reply of a worker fed with the mesh's centres and the messages `script(post, sort)` posts
const sortsOf = (mesh, count, script) => new Promise((resolve) => {
  const w = gs.createSortWorker(total, false, false, true, false);
  const replies = [];
  let expected = 0;
  w.onmessage = (e) => {
    if (!e.data.sortDone) return;
    replies.push({ count: e.data.splatRenderCount, list: Uint32Array.from(e.data.sortedIndexes) });
    if (replies.length === expected) { const uploaded = w.uploadedSplatCount; w.terminate(); resolve({ replies, uploaded }); }
  };
  w.postMessage({ centers: mesh.getIntegerCenters(0, count - 1, true).buffer, range: { from: 0, to: count - 1, count } });
  const sort = (n) => { expected++; w.postMessage({ sort: { modelViewProj: a.sortMvp, splatRenderCount: n, splatSortCount: n, usePrecomputedDistances: false } }); };
  script((msg) => w.postMessage(msg), sort, w);
});

async function main() {
  const out = {};
  const edited = meshOf([0, 1, 2]), fresh = meshOf([0, 2]);
  frameOf(edited, Uint32Array.from({ length: total }, (_, i) => i), total);   // a draw of the three scenes first
  const before = a.dynamic ? null : edited.getIntegerCenters(0, total - 1, true);
  const r = edited.removeScenes([1]);
  out.edited = r.edited;
  out.ranges = r.ranges; out.sceneRemap = r.sceneRemap;
  out.stateEqual = stateOf(edited) === stateOf(fresh);
  out.treeGone = edited.getSplatTree() === null;
  out.regionCovers = edited.maxSplatDistanceFromSceneCenter >= fresh.maxSplatDistanceFromSceneCenter && fresh.maxSplatDistanceFromSceneCenter > 0;
  let order = Uint32Array.from(a.order), listEqual = true, queued = true;
  if (!a.dynamic) {
    // (the worker still holds the three scenes' centres when the first sort starts: they were read before the removal)
    const threeScenes = { getIntegerCenters: () => before };
    const A = await sortsOf(threeScenes, total, (post, sort, w) => {
      sort(total);
      queued = w._busy === true;                              // the sort is in flight: what follows waits in the queue
      post({ remove: { ranges: r.ranges, sceneRemap: r.sceneRemap } });
      sort(left);
      queued = queued && w._queue.length === 2;
    });
    const B = await sortsOf(fresh, left, (post, sort) => sort(left));
    const la = A.replies[1].list, lb = B.replies[0].list;
    listEqual = A.replies.length === 2 && A.replies[0].count === total && A.replies[1].count === left && A.uploaded === left &&
                Buffer.compare(Buffer.from(la.buffer), Buffer.from(lb.buffer)) === 0;
    order = la;
  }
  out.listEqual = listEqual; out.queued = queued;
  const fa = frameOf(edited, order, left), fb = frameOf(fresh, order, left);
  out.frameEqual = Buffer.compare(fa, fb) === 0 && fa.some((v) => v !== 0);
  // removing what is left but one, then the last: counts go to zero without a device mesh to edit
  edited.removeScenes([0]);
  out.oneLeft = edited.getSceneCount() === 1 && edited.getSplatCount() === buffers[2].max;
  const single = meshOf([2]);
  const one = Uint32Array.from({ length: buffers[2].max }, (_, i) => i);
  out.oneLeftFrameEqual = Buffer.compare(frameOf(edited, one, one.length), frameOf(single, one, one.length)) === 0;
  edited.removeScenes([0]);
  out.noneLeft = edited.getSceneCount() === 0 && edited.getSplatCount() === 0 && edited.visible === false;
  // the fall-back: the last buffer is still loading, so the device mesh is built afresh from the buffers that stay
  buffers[2].splatCount = buffers[2].max - 57;
  const loading = meshOf([0, 1, 2]), loadingFresh = meshOf([0, 2]);
  const r2 = loading.removeScenes([1]);
  const part = left - 57, partOrder = Uint32Array.from({ length: part }, (_, i) => part - 1 - i);
  out.fallbackEdited = r2.edited;
  out.fallbackStateEqual = stateOf(loading) === stateOf(loadingFresh);
  out.fallbackFrameEqual = Buffer.compare(frameOf(loading, partOrder, part), frameOf(loadingFresh, partOrder, part)) === 0;
  let threw = false;
  try { loading.removeScenes([5]); } catch (e) { threw = /Invalid scene index/.test(e.message); }
  out.badIndexRefused = threw;
  console.log(JSON.stringify(out));
  for (const m of [edited, fresh, single, loading, loadingFresh]) m.dispose();
}
main().catch((e) => { console.error(e); process.exit(1); });
