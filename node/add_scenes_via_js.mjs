// Test driver: adding scenes to a live drop-in mesh and sort worker.  usage: node add_scenes_via_js.mjs <in.json>
// in.json: {scenes: [{centers, cov, rgba (plain arrays), position}] (three), dynamic, order (a draw order of all splats), width,
//           height, focal, matrixWorld, view, proj, sortMvp}
// 1. the addon: meshResize / sorterResize on a mesh and sorter that hold two scenes, then the third - against a mesh and sorter
//    of the full capacity that received the same three uploads; refusals throw and change nothing.
// 2. SplatMesh.addScenes of the drop-in (node/SplatMesh.mjs) on a two-scene mesh against a drop-in mesh built from all three
//    buffers at once: host bookkeeping, the frame and the list of a worker (a dynamic-mode one in the dynamic run, with scene
//    indexes and transforms) that received `sort`, `resize`, the `centers` message of the new range only and `sort` back to
//    back, so that the resize waits in the queue behind the sort in flight; the same through a worker in shared-memory mode,
//    whose `sortResized` reply carries the grown arrays.  Before that one scene becomes two (the add that first gives the device
//    mesh scene indexes).  Then removeScenes takes the added scene out again on the device.
// 3. the fall-backs: a buffer of another SH degree, a buffer still loading and a scene beyond Constants.MaxScenes take the full
//    build, and the mesh ends as one built from all buffers at once does - the same frame, or the same refusal.
// stdout: one JSON line.
import fs from 'fs';
import { createRequire } from 'module';
import * as THREE from 'three';
import { SplatMesh } from './SplatMesh.mjs';
const require = createRequire(import.meta.url);
const gs = require('./gsplat.js');
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

class StandInBuffer {                                       // the methods the drop-in calls on a reference SplatBuffer
  constructor(scene, degree = 0) {
    this.s = scene;
    this.max = scene.centers.length / 3;
    this.degree = degree;
    Object.assign(this, { splatCount: this.max, compressionLevel: 0, sceneCenter: new THREE.Vector3(0, 0, 0),
                          minSphericalHarmonicsCoeff: -1.5, maxSphericalHarmonicsCoeff: 1.5 });
  }
  getSplatCount() { return this.splatCount; }
  getMaxSplatCount() { return this.max; }
  getMinSphericalHarmonicsDegree() { return this.degree; }
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
  fillSphericalHarmonicsArray(out, degree, transform, from = 0, to = this.splatCount - 1, dest = 0) {   // (half bits of small values)
    const n = [0, 9, 24][degree];
    for (let i = from; i <= to; i++) for (let k = 0; k < n; k++) out[(i - from + dest) * n + k] = gs.toHalfFloat(((i * 7 + k * 3) % 11 - 5) / 16);
  }
}

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);
const buffers = a.scenes.map((s) => new StandInBuffer(s)), options = a.scenes.map((s) => ({ position: s.position }));
const meshOf = (bufs, opts, degree = 0) => {
  const mesh = new SplatMesh(0, !!a.dynamic, false, false, 1, false, true, false, 1024, 0, degree, 1.0, 0.3);
  mesh.build(bufs, opts, true, false);
  return mesh;
};
const frameOf = (mesh, order, count) => {
  mesh.updateRenderIndexes(order, count);
  mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
  return Buffer.from(mesh.renderFrame(camera).data);
};
const stateOf = (m, bufs = buffers) => JSON.stringify([m.getSplatCount(), m.getSplatCount(true), m.getMaxSplatCount(), m.getSceneCount(),
  m.lastBuildSplatCount, m.lastBuildMaxSplatCount, m.lastBuildSceneCount, m.lastBuildScenes.map((sc) => bufs.indexOf(sc.splatBuffer)), m.sceneOptions,
  m.globalSplatIndexToLocalSplatIndexMap, m.globalSplatIndexToSceneIndexMap, m.scenes.map((sc) => Array.from(sc.transform.elements)),
  m.calculatedSceneCenter.toArray(), m.visible, m.minSphericalHarmonicsDegree, m.core.maxSplatCount, m.getSplatDataTextures().maxSplatCount]);
const same = (x, y) => Buffer.compare(Buffer.from(x.buffer, x.byteOffset, x.byteLength), Buffer.from(y.buffer, y.byteOffset, y.byteLength)) === 0;
const sizes = buffers.map((b) => b.max), two = sizes[0] + sizes[1], total = two + sizes[2];
const threw = (call, pattern) => { try { call(); } catch (e) { return pattern.test(String(e && e.message)); } return false; };

// every sortDone reply of a worker of capacity `capacity` fed by `script(post, sort, worker)`
const sortsOf = (capacity, script) => new Promise((resolve) => {
  const w = gs.createSortWorker(capacity, false, false, true, !!a.dynamic);
  const replies = [];
  let expected = 0, resized = null;
  w.onmessage = (e) => {
    if (e.data.sortResized) resized = e.data.maxSplatCount;
    if (!e.data.sortDone) return;
    replies.push({ count: e.data.splatRenderCount, list: Uint32Array.from(e.data.sortedIndexes) });
    if (replies.length === expected) {
      const state = { replies, uploaded: w.uploadedSplatCount, maxSplatCount: w.maxSplatCount, resized, hostBytes: w.sortedIndexesBuffer.byteLength };
      w.terminate();
      resolve(state);
    }
  };
  const sort = (n) => {
    expected++;
    w.postMessage({ sort: { modelViewProj: a.sortMvp, splatRenderCount: n, splatSortCount: n, usePrecomputedDistances: false,
                            transforms: a.dynamic ? sceneTransforms : undefined } });
  };
  script((msg) => w.postMessage(msg), sort, w);
});
let sceneTransforms = null, sceneOf = null;                 // the three scenes' matrices and scene indexes (a dynamic worker's inputs)
const centersMessage = (centers, from, count) => ({ centers: centers.buffer.slice(centers.byteOffset, centers.byteOffset + centers.byteLength),
                                                    sceneIndexes: Uint32Array.from(sceneOf.slice(from, from + count)),
                                                    range: { from, to: from + count - 1, count } });

// A worker in shared-memory mode, one message at a time: the two scenes, a sort, `resize` - whose reply carries the grown shared
// arrays, which are the ones written from then on - the new range, a sort of everything from an explicit identity list.
const sharedRun = (all, added) => new Promise((resolve) => {
  const w = gs.createSortWorker(two, true, false, true, !!a.dynamic);
  const state = {};
  const sort = (n) => {
    const indexes = new Uint32Array(w.indexesToSortBuffer);
    for (let i = 0; i < n; i++) indexes[i] = i;
    new Float32Array(w.transformsBuffer).set(sceneTransforms);
    w.postMessage({ sort: { modelViewProj: a.sortMvp, splatRenderCount: n, splatSortCount: n, usePrecomputedDistances: false } });
  };
  let sorted = 0;
  w.onmessage = (e) => {
    if (e.data.sortSetupPhase1Complete) {
      w.postMessage(centersMessage(all.subarray(0, 4 * two), 0, two));
      sort(two);
    } else if (e.data.sortResized) {
      const shared = typeof SharedArrayBuffer === 'undefined' || e.data.sortedIndexesBuffer instanceof SharedArrayBuffer;
      state.resized = e.data.maxSplatCount === total && shared && e.data.sortedIndexesBuffer === w.sortedIndexesBuffer &&
                      e.data.indexesToSortBuffer === w.indexesToSortBuffer && e.data.precomputedDistancesBuffer === w.precomputedDistancesBuffer &&
                      [e.data.sortedIndexesBuffer, e.data.indexesToSortBuffer, e.data.precomputedDistancesBuffer].every((b) => b.byteLength >= total * 4);
      w.postMessage(centersMessage(added.centers, added.from, added.count));
      sort(total);
    } else if (e.data.sortDone && sorted++ === 0) {
      state.first = e.data.splatRenderCount;
      w.postMessage({ resize: { maxSplatCount: total } });
    } else if (e.data.sortDone) {
      state.list = Uint32Array.from(new Uint32Array(w.sortedIndexesBuffer, 0, e.data.splatRenderCount));
      state.maxSplatCount = w.maxSplatCount;
      w.terminate();
      resolve(state);
    }
  };
});

async function main() {
  const out = {};
  const order = Uint32Array.from(a.order);

  // ---- 1. the addon calls ----------------------------------------------------------------------------------------------------
  {
    const f32 = (k, name) => Float32Array.from(a.scenes[k][name]), u8 = (k) => Uint8Array.from(a.scenes[k].rgba);
    const grown = new gs.SplatMeshHIP(two), full = new gs.SplatMeshHIP(total);
    const put = (mesh, k, at) => mesh.build(f32(k, 'centers'), f32(k, 'cov'), u8(k), null, at);
    put(grown, 0, 0); put(grown, 1, sizes[0]);
    out.addonUploadRefused = threw(() => put(grown, 2, two), /max_splat_count/);
    out.addonRefusals = threw(() => grown.resize(two - 1), /uploaded count/) && threw(() => grown.resize(0), /max_splat_count == 0/) && grown.maxSplatCount === two;
    grown.resize(total);
    put(grown, 2, two);
    [0, 1, 2].reduce((at, k) => { put(full, k, at); return at + sizes[k]; }, 0);
    const positions = [new Uint32Array(total), new Uint32Array(total)];
    gs.addon.meshStoragePositions(grown.handle, positions[0]);
    gs.addon.meshStoragePositions(full.handle, positions[1]);
    out.addonMeshEqual = grown.maxSplatCount === total && same(positions[0], positions[1]);
    grown.dispose(); full.dispose();
    const sorter = gs.addon.sorterCreate(grown.ctx.handle, two, 1, 16);
    out.addonSorterRefusal = threw(() => gs.addon.sorterResize(sorter, 0), /max_splat_count == 0/);
    gs.addon.sorterResize(sorter, total);
    gs.addon.sorterResize(sorter, total);                   // the capacity it has: nothing happens
    gs.addon.sorterDestroy(sorter);
  }

  // ---- 2. SplatMesh.addScenes --------------------------------------------------------------------------------------------------
  // one scene becomes two: the Viewer's usual case, and the add that gives the device mesh its scene-index plane
  {
    const solo = meshOf(buffers.slice(0, 1), options.slice(0, 1)), both = meshOf(buffers.slice(0, 2), options.slice(0, 2));
    frameOf(solo, Uint32Array.from({ length: sizes[0] }, (_, i) => i), sizes[0]);
    const r1 = solo.addScenes([buffers[1]], [options[1]]);
    out.soloEdited = r1.edited === true && r1.from === sizes[0] && r1.count === sizes[1] && r1.sceneIndexes.every((v) => v === 1);
    out.soloStateEqual = stateOf(solo) === stateOf(both);
    const mixed = Uint32Array.from({ length: two }, (_, i) => (i * 7) % two);      // (7 and 557 are coprime: a permutation)
    const fs1 = frameOf(solo, mixed, two);
    out.soloFrameEqual = Buffer.compare(fs1, frameOf(both, mixed, two)) === 0 && fs1.some((v) => v !== 0);
    solo.dispose(); both.dispose();
  }
  const edited = meshOf(buffers.slice(0, 2), options.slice(0, 2)), fresh = meshOf(buffers, options);
  frameOf(edited, Uint32Array.from({ length: two }, (_, i) => i), two);        // a draw of the two scenes first
  const resident = edited.getSplatCount();
  const scenesBefore = edited.scenes.slice();
  const r = edited.addScenes([buffers[2]], [options[2]]);
  out.edited = r.edited === true && r.from === two && r.to === total - 1 && r.count === sizes[2] && resident === two;
  out.scenesKept = scenesBefore.every((sc, k) => edited.scenes[k] === sc) && edited.getSceneCount() === 3;
  out.stateEqual = stateOf(edited) === stateOf(fresh);
  out.treeGone = edited.getSplatTree() === null;
  out.regionCovers = edited.maxSplatDistanceFromSceneCenter >= fresh.maxSplatDistanceFromSceneCenter && fresh.maxSplatDistanceFromSceneCenter > 0;
  const all = fresh.getIntegerCenters(0, total - 1, true);
  out.replyCenters = same(r.centers, all.subarray(4 * two));
  sceneOf = fresh.globalSplatIndexToSceneIndexMap;
  sceneTransforms = new Float32Array(16 * 3);
  fresh.fillTransformsArray(sceneTransforms);
  out.replySceneIndexes = r.sceneIndexes.length === sizes[2] && r.sceneIndexes.every((v) => v === 2);
  let list = order;
  {
    let queued = false;
    const A = await sortsOf(two, (post, sort, w) => {
      post(centersMessage(all.subarray(0, 4 * two), 0, two));
      sort(two);
      queued = w._busy === true;                              // the sort is in flight: what follows waits in the queue
      post({ resize: { maxSplatCount: edited.getMaxSplatCount() } });
      post(centersMessage(r.centers, r.from, r.count));       // the new range only
      sort(total);
      queued = queued && w._queue.length === 3;
    });
    const B = await sortsOf(total, (post, sort) => { post(centersMessage(all, 0, total)); sort(total); });
    out.queued = queued;
    out.workerState = A.maxSplatCount === total && A.resized === total && A.uploaded === total && A.hostBytes >= total * 4;
    out.listEqual = A.replies.length === 2 && A.replies[0].count === two && A.replies[1].count === total && same(A.replies[1].list, B.replies[0].list);
    list = A.replies[1].list;
    const S = await sharedRun(all, r);
    out.sharedResized = S.resized === true && S.first === two && S.maxSplatCount === total;
    out.sharedListEqual = same(S.list, list);
  }
  const fa = frameOf(edited, list, total), fb = frameOf(fresh, list, total);
  out.frameEqual = Buffer.compare(fa, fb) === 0 && fa.some((v) => v !== 0);
  // the added scene goes again, on the device
  const gone = edited.removeScenes([2]);
  const pair = meshOf(buffers.slice(0, 2), options.slice(0, 2));
  const firstTwo = Uint32Array.from({ length: two }, (_, i) => two - 1 - i);
  out.removedAgain = gone.edited === true && Buffer.compare(frameOf(edited, firstTwo, two), frameOf(pair, firstTwo, two)) === 0;
  // ... and comes back (a removal keeps the capacity: this resize is to the capacity the device mesh still has)
  out.addedAgain = edited.addScenes([buffers[2]], [options[2]]).edited === true && Buffer.compare(frameOf(edited, list, total), fb) === 0;

  // ---- 3. the fall-backs -------------------------------------------------------------------------------------------------------
  // a mesh of SH degree 1 whose new buffer has none: the build would choose degree 0, the planes cannot stay
  const sh = buffers.map((b, k) => new StandInBuffer(a.scenes[k], k === 2 ? 0 : 1));
  const shEdited = meshOf(sh.slice(0, 2), options.slice(0, 2), 1), shFresh = meshOf(sh, options, 1);
  const r2 = shEdited.addScenes([sh[2]], [options[2]]);
  out.degreeFallback = r2.edited === false && r2.from === 0 && r2.count === total && shEdited.minSphericalHarmonicsDegree === 0;
  out.degreeStateEqual = stateOf(shEdited, sh) === stateOf(shFresh, sh);
  out.degreeFrameEqual = Buffer.compare(frameOf(shEdited, order, total), frameOf(shFresh, order, total)) === 0;
  // a buffer that is still loading
  buffers[2].splatCount = buffers[2].max - 57;
  const loading = meshOf(buffers.slice(0, 2), options.slice(0, 2)), loadingFresh = meshOf(buffers, options);
  const r3 = loading.addScenes([buffers[2]], [options[2]]);
  const part = total - 57, partOrder = Uint32Array.from({ length: part }, (_, i) => part - 1 - i);
  out.loadingFallback = r3.edited === false && stateOf(loading) === stateOf(loadingFresh) &&
                        Buffer.compare(frameOf(loading, partOrder, part), frameOf(loadingFresh, partOrder, part)) === 0;
  buffers[2].splatCount = buffers[2].max;
  // a 33rd scene: what a build of all 33 buffers does - the device holds Constants.MaxScenes scene indexes and refuses it
  const tiny = (k) => new StandInBuffer({ centers: a.scenes[0].centers.slice(3 * k, 3 * k + 3), cov: a.scenes[0].cov.slice(6 * k, 6 * k + 6),
                                          rgba: a.scenes[0].rgba.slice(4 * k, 4 * k + 4) });
  const many = Array.from({ length: gs.Constants.MaxScenes + 1 }, (_, k) => tiny(k)), manyOptions = many.map(() => ({}));
  const crowded = meshOf(many.slice(0, 31), manyOptions.slice(0, 31));
  out.sceneLimitInPlace = crowded.addScenes([many[31]], [{}]).edited === true && crowded.getSceneCount() === 32;
  const crowdedFresh = meshOf(many.slice(0, 32), manyOptions.slice(0, 32));
  const few = Uint32Array.from({ length: 32 }, (_, i) => i);
  out.sceneLimitFrameEqual = Buffer.compare(frameOf(crowded, few, 32), frameOf(crowdedFresh, few, 32)) === 0;
  let builtError = null, addedError = null;
  try { meshOf(many, manyOptions).dispose(); } catch (e) { builtError = String(e && e.message); }
  try { out.sceneLimitFallback = crowded.addScenes([many[32]], [{}]).edited === false; } catch (e) { addedError = String(e && e.message); }
  out.sceneLimitAsBuild = builtError === addedError && (builtError !== null || out.sceneLimitFallback === true);
  out.sceneLimitError = builtError;
  console.log(JSON.stringify(out));
  for (const m of [edited, fresh, pair, shEdited, shFresh, loading, loadingFresh, crowded, crowdedFresh]) m.dispose();
}
main().catch((e) => { console.error(e); process.exit(1); });
