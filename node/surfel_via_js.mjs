// Test driver: one SplatRenderMode.TwoD frame through the drop-in (node/SplatMesh.mjs).
// usage: node surfel_via_js.mjs <in.json> <outDir>
// in.json: {centers, scales, rotations (x, y, z, w), rgba (plain arrays, n splats), sceneCenter, order, width, height, focal,
//           matrixWorld, view, proj}
// A stand-in buffer with the methods the drop-in calls on a reference SplatBuffer; its fillSplatScaleRotationArray and
// getSplatScaleAndRotation apply the scaleOverride they are handed the way SplatBuffer.js does (a component that is not undefined
// replaces the scale's).  -> <outDir>/frame.u8, <outDir>/records.u32 (the addon's test hook meshDebugRecords2D), and on stdout
// {scaleZ: what getSplatScaleAndRotation reports for splat 0, uploadedScaleZ: the z the fill was asked to store, refusesOther}.
import fs from 'fs';
import path from 'path';
import * as THREE from 'three';
import { SplatMesh, SplatRenderMode } from './SplatMesh.mjs';
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8')), outDir = process.argv[3];
const n = a.centers.length / 3;
const seen = { uploadedScaleZ: null };

class StandInBuffer {
  constructor() {
    Object.assign(this, { compressionLevel: 0, sceneCenter: new THREE.Vector3().fromArray(a.sceneCenter),
                          minSphericalHarmonicsCoeff: -1.5, maxSphericalHarmonicsCoeff: 1.5 });
  }
  getSplatCount() { return n; }
  getMaxSplatCount() { return n; }
  getMinSphericalHarmonicsDegree() { return 0; }
  _copy(src, width, out, from = 0, to = n - 1, dest = 0) {
    for (let i = from; i <= to; i++) for (let k = 0; k < width; k++) out[(i - from + dest) * width + k] = src[i * width + k];
  }
  fillSplatCenterArray(out, transform, from, to, dest) { this._copy(a.centers, 3, out, from, to, dest); }
  fillSplatCovarianceArray() { throw new Error('a SplatRenderMode.TwoD mesh must not ask for covariances'); }
  fillSplatColorArray(out, minimumAlpha, from, to, dest) { this._copy(a.rgba, 4, out, from, to, dest); }
  fillSplatScaleRotationArray(outScale, outRotation, transform, from = 0, to = n - 1, dest = 0, level, scaleOverride) {
    this._copy(a.scales, 3, outScale, from, to, dest);
    this._copy(a.rotations, 4, outRotation, from, to, dest);
    ['x', 'y', 'z'].forEach((axis, k) => {
      if (scaleOverride && scaleOverride[axis] !== undefined) for (let i = from; i <= to; i++) outScale[(i - from + dest) * 3 + k] = scaleOverride[axis];
    });
    seen.uploadedScaleZ = scaleOverride ? scaleOverride.z : undefined;
  }
  getSplatScaleAndRotation(index, outScale, outRotation, transform, scaleOverride) {
    outScale.set(a.scales[3 * index], a.scales[3 * index + 1], a.scales[3 * index + 2]);
    for (const axis of ['x', 'y', 'z']) if (scaleOverride && scaleOverride[axis] !== undefined) outScale[axis] = scaleOverride[axis];
    outRotation.set(a.rotations[4 * index], a.rotations[4 * index + 1], a.rotations[4 * index + 2], a.rotations[4 * index + 3]);
  }
}

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);

let refusesOther = false;
try { new SplatMesh(7); } catch (e) { refusesOther = true; }
// halfPrecisionCovariancesOnGPU = true on purpose: 2D mode keeps fp32 scales and rotations whatever it says
const mesh = new SplatMesh(SplatRenderMode.TwoD, false, false, true, 1, false, true, false, 1024, 0, 0, 1.0, 0.3);
mesh.build([new StandInBuffer()], [{}], true, true);
mesh.updateRenderIndexes(Uint32Array.from(a.order), n);
mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
fs.writeFileSync(path.join(outDir, 'frame.u8'), Buffer.from(mesh.renderFrame(camera).data));
fs.writeFileSync(path.join(outDir, 'records.u32'), Buffer.from(mesh.core.debugRecords2D().buffer));
const scale = new THREE.Vector3(), rotation = new THREE.Quaternion();
mesh.getSplatScaleAndRotation(0, scale, rotation);
console.log(JSON.stringify({ scaleZ: scale.z, scaleX: scale.x, uploadedScaleZ: seen.uploadedScaleZ, refusesOther }));
mesh.dispose();
