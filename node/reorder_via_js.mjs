// Test driver: a progressive load through the drop-in (node/SplatMesh.mjs) that ends with the fold of its Morton runs.
// usage: node reorder_via_js.mjs <in.json> <outDir>
// in.json: {centers, cov, rgba (plain arrays, n splats), sceneCenter, counts: [splats loaded at every build, the last one final], order,
//           width, height, focal, matrixWorld, view, proj}
// Three meshes over the same stand-in buffer (the methods the drop-in calls on a reference SplatBuffer; its splat count grows from
// build to build): `folded` builds it in counts.length builds with foldRunsAtFinalBuild = true, `pieces` does the same with the
// property at its default, `once` builds the finished buffer in one final build.  Of each: the storage position of every splat
// (the addon's test hook meshStoragePositions) -> <outDir>/<name>.pos.u32 and the frame -> <outDir>/<name>.u8.
import fs from 'fs';
import path from 'path';
import { createRequire } from 'module';
import * as THREE from 'three';
import { SplatMesh } from './SplatMesh.mjs';
const { addon } = createRequire(import.meta.url)('./gsplat.js');
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8')), outDir = process.argv[3];
const n = a.centers.length / 3;

class StandInBuffer {
  constructor() {
    Object.assign(this, { splatCount: 0, compressionLevel: 0, sceneCenter: new THREE.Vector3().fromArray(a.sceneCenter),
                          minSphericalHarmonicsCoeff: -1.5, maxSphericalHarmonicsCoeff: 1.5 });
  }
  getSplatCount() { return this.splatCount; }
  getMaxSplatCount() { return n; }
  getMinSphericalHarmonicsDegree() { return 0; }
  _copy(src, width, out, from = 0, to = this.splatCount - 1, dest = 0) {
    for (let i = from; i <= to; i++) for (let k = 0; k < width; k++) out[(i - from + dest) * width + k] = src[i * width + k];
  }
  fillSplatCenterArray(out, transform, from, to, dest) { this._copy(a.centers, 3, out, from, to, dest); }
  fillSplatCovarianceArray(out, transform, from, to, dest) { this._copy(a.cov, 6, out, from, to, dest); }
  fillSplatColorArray(out, minimumAlpha, from, to, dest) { this._copy(a.rgba, 4, out, from, to, dest); }
}

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);

const load = (name, counts, fold) => {
  const mesh = new SplatMesh(0, false, false, false, 1, false, true, false, 1024, 0, 0, 1.0, 0.3);
  const defaultOff = mesh.foldRunsAtFinalBuild === false;
  if (fold) mesh.foldRunsAtFinalBuild = true;
  const buffer = new StandInBuffer();
  let loading = null;
  counts.forEach((count, k) => {
    buffer.splatCount = count;
    mesh.build([buffer], [{}], true, k === counts.length - 1);
    if (k === 0 && counts.length > 1) loading = mesh.reorderScenes().length;       // a buffer still loading is skipped
  });
  const pos = new Uint32Array(n);
  addon.meshStoragePositions(mesh.core.handle, pos);
  fs.writeFileSync(path.join(outDir, `${name}.pos.u32`), Buffer.from(pos.buffer));
  mesh.updateRenderIndexes(Uint32Array.from(a.order), n);
  mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
  fs.writeFileSync(path.join(outDir, `${name}.u8`), Buffer.from(mesh.renderFrame(camera).data));
  const again = mesh.reorderScenes();                      // one run by now, or five: the call folds what is there
  return { mesh, defaultOff, loading, again };
};

const out = {};
for (const [name, counts, fold] of [['folded', a.counts, true], ['pieces', a.counts, false], ['once', [n], false]]) {
  const r = load(name, counts, fold);
  out[name] = { defaultOff: r.defaultOff, skippedWhileLoading: r.loading, spansAtTheEnd: r.again };
  if (name === 'pieces') {                                 // reorderScenes by hand does what the property does at the final build
    const pos = new Uint32Array(n);
    addon.meshStoragePositions(r.mesh.core.handle, pos);
    fs.writeFileSync(path.join(outDir, 'pieces_folded_by_hand.pos.u32'), Buffer.from(pos.buffer));
  }
  r.mesh.dispose();
}
console.log(JSON.stringify(out));
