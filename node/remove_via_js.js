// Removes the middle one of three scenes through the addon (meshRemove) and through the sort worker's `remove` message (test
// driver).  usage: node remove_via_js.js <in.bin> <out.bin>
// in.bin: uint32 header {n0, n1, n2, width, height, 0, 0, 0}, then centers F32[3n], cov F32[6n], rgba U8[4n], order U32[n0 + n2],
// intCenters I32[4n], modelView F32[16], proj F32[16], camPos F32[3], focal F32[2], sortMvp F32[16]   (n = n0 + n1 + n2)
// out.bin: the edited mesh's frame U8[4 * width * height], then the edited worker's sorted list U32[n0 + n2]; stdout: one JSON line
// {meshEqual, sorterEqual}: the same through a fresh mesh / a fresh worker that only ever saw the two scenes that stay
'use strict';
const fs = require('fs');
const gs = require('./gsplat.js');
const [inPath, outPath] = process.argv.slice(2);
const buf = fs.readFileSync(inPath);
const ab = buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength);
const [n0, n1, n2, width, height] = new Uint32Array(ab, 0, 8);
const n = n0 + n1 + n2, left = n0 + n2;
let off = 32;
const take = (Type, count) => { const a = new Type(ab.slice(off, off + count * Type.BYTES_PER_ELEMENT)); off += count * Type.BYTES_PER_ELEMENT; return a; };
const centers = take(Float32Array, 3 * n), cov = take(Float32Array, 6 * n), rgba = take(Uint8Array, 4 * n), order = take(Uint32Array, left);
const intCenters = take(Int32Array, 4 * n);
const modelView = take(Float32Array, 16), proj = take(Float32Array, 16), camPos = take(Float32Array, 3), focal = take(Float32Array, 2);
const sortMvp = take(Float32Array, 16);
const spans = [[0, n0], [n0, n1], [n0 + n1, n2]];

function meshOf(which) {                                    // every scene is one upload, one behind the other
  const mesh = new gs.SplatMeshHIP(n, { sphericalHarmonicsDegree: 0 });
  let at = 0;
  for (const k of which) {
    const [b, c] = spans[k];
    mesh.build(centers.subarray(3 * b, 3 * (b + c)), cov.subarray(6 * b, 6 * (b + c)), rgba.subarray(4 * b, 4 * (b + c)), null, at);
    at += c;
  }
  mesh.updateUniforms({ x: width, y: height }, focal[0], focal[1], false, 1.0, 1.0);
  mesh.setCameraMatrices(modelView, proj, camPos);
  return mesh;
}
function frameOf(mesh) {
  mesh.updateRenderIndexes(order, left);
  const { pixels } = mesh.render();
  return Buffer.from(pixels.buffer, pixels.byteOffset, pixels.byteLength);
}
const edited = meshOf([0, 1, 2]), fresh = meshOf([0, 2]);
edited.updateRenderIndexes(new Uint32Array(n).map((_, i) => i), n);
edited.render();
edited.remove([[n0, n1]]);
let threw = false;
try { edited.remove([[1, 1]]); } catch (e) { threw = /Morton run/.test(String(e.message)); }   // a border inside a run is refused
const frame = frameOf(edited);
const meshEqual = threw && edited.getSplatCount() === left && Buffer.compare(frame, frameOf(fresh)) === 0;
edited.dispose();
fresh.dispose();

function workerOf(which, then) {
  const w = gs.createSortWorker(n, false, false, true, false);
  w.synchronous = true;
  const replies = [];
  w.onmessage = (e) => { if (e.data.sortDone) replies.push(e.data); };
  let at = 0;
  for (const k of which) {
    const [b, c] = spans[k];
    w.postMessage({ centers: intCenters.slice(4 * b, 4 * (b + c)).buffer, range: { from: at, to: at + c - 1, count: c } });
    at += c;
  }
  const sort = (count) => w.postMessage({ sort: { modelViewProj: Array.from(sortMvp), splatRenderCount: count, splatSortCount: count, usePrecomputedDistances: false } });
  if (which.length === 3) {                                 // a sort before, the removal, the sort after: in posting order
    sort(n);
    w.postMessage({ remove: { ranges: [[n0, n1]] } });
  }
  sort(left);
  setImmediate(() => { const last = replies[replies.length - 1]; const count = w.uploadedSplatCount; w.terminate(); then(last, count, replies.length); });
}
workerOf([0, 1, 2], (a, countA, repliesA) => workerOf([0, 2], (b) => {
  const la = Buffer.from(a.sortedIndexes.buffer, a.sortedIndexes.byteOffset, a.sortedIndexes.byteLength);
  const lb = Buffer.from(b.sortedIndexes.buffer, b.sortedIndexes.byteOffset, b.sortedIndexes.byteLength);
  const sorterEqual = repliesA === 2 && countA === left && a.splatRenderCount === left && Buffer.compare(la, lb) === 0;
  fs.writeFileSync(outPath, Buffer.concat([frame, la]));
  console.log(JSON.stringify({ meshEqual, sorterEqual }));
}));
