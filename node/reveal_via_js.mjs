// Test driver: a progressive load with the scene reveal through the drop-in (node/SplatMesh.mjs).  usage: node reveal_via_js.mjs <in.json> <outDir>
// in.json: {centers, cov, rgba (plain arrays, n splats), sceneCenter, builds: [{count, finalBuild, frames, order}], mode, width, height, focal,
//           matrixWorld, view, proj, boxScene: {position, scale}}
// The splat buffer is a stand-in with the methods the drop-in calls on a reference SplatBuffer (the fills copy the arrays; a
// transform moves the centres as THREE.Vector3.applyMatrix4 does); its splat count grows from build to build, as a progressive
// load's does.  After every build and every frame the state; after the last frame of every build the frame -> <outDir>/shot<k>.u8.
// Then: a mesh under SceneRevealMode.Instant and one whose updateVisibleRegionFadeDistance is never called (instant.u8, uncalled.u8),
// and computeBoundingBox of the mesh and of a second mesh whose scene has a static transform.
import fs from 'fs';
import path from 'path';
import * as THREE from 'three';
import { SplatMesh, SceneRevealMode } from './SplatMesh.mjs';
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
  fillSplatCenterArray(out, transform, from = 0, to = this.splatCount - 1, dest = 0) {
    const v = new THREE.Vector3();
    for (let i = from; i <= to; i++) {
      v.set(a.centers[3 * i], a.centers[3 * i + 1], a.centers[3 * i + 2]);
      if (transform) v.applyMatrix4(transform);
      out[(i - from + dest) * 3] = v.x; out[(i - from + dest) * 3 + 1] = v.y; out[(i - from + dest) * 3 + 2] = v.z;
    }
  }
  fillSplatCovarianceArray(out, transform, from, to, dest) { this._copy(a.cov, 6, out, from, to, dest); }
  fillSplatColorArray(out, minimumAlpha, from, to, dest) { this._copy(a.rgba, 4, out, from, to, dest); }
}

const camera = { matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
camera.matrixWorldInverse = new THREE.Matrix4().fromArray(a.view);
const state = (m) => [m.maxSplatDistanceFromSceneCenter, m.visibleRegionBufferRadius, m.visibleRegionRadius, m.visibleRegionFadeStartRadius,
                      m.visibleRegionChanging, m._region.shaderFadeInComplete];
const draw = (mesh, b, file) => {
  mesh.updateRenderIndexes(Uint32Array.from(b.order), b.count);
  mesh.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
  fs.writeFileSync(path.join(outDir, file), Buffer.from(mesh.renderFrame(camera).data));
};
// one progressive load; perFrame(mesh) is the Viewer's per-frame call (or nothing)
const load = (perFrame, shots) => {
  const mesh = new SplatMesh(0, false, false, false, 1, false, true, false, 1024, 0, 0, 1.0, 0.3);
  const buffer = new StandInBuffer(), rows = [];
  a.builds.forEach((b, k) => {
    buffer.splatCount = b.count;
    mesh.build([buffer], [{}], true, b.finalBuild);
    rows.push(mesh.calculatedSceneCenter.toArray().concat(state(mesh)));
    for (let f = 0; f < b.frames; f++) { perFrame(mesh); rows.push(state(mesh)); }
    if (shots) draw(mesh, b, shots(k));
  });
  return { mesh, rows };
};

const out = {};
const main = load((mesh) => mesh.updateVisibleRegionFadeDistance(a.mode), (k) => `shot${k}.u8`);
out.rows = main.rows;
const box = (b) => ({ min: b.min.toArray(), max: b.max.toArray() });
out.boxPlain = box(main.mesh.computeBoundingBox());
out.boxTransformed = box(main.mesh.computeBoundingBox(true));
out.boxScene0 = box(main.mesh.computeBoundingBox(false, 0));
try { main.mesh.computeBoundingBox(false, 1); out.badIndex = null; } catch (e) { out.badIndex = e.message; }
const last = a.builds[a.builds.length - 1];
const instant = load((mesh) => mesh.updateVisibleRegionFadeDistance(SceneRevealMode.Instant), null);
draw(instant.mesh, last, 'instant.u8');
const uncalled = load(() => {}, null);
draw(uncalled.mesh, last, 'uncalled.u8');
out.uncalledChanging = uncalled.mesh.visibleRegionChanging;
// a static scene transform: the transformed box is what the device stores, the plain one comes from the host fill
const moved = new SplatMesh(0, false, false, false, 1, false, true, false, 1024, 0, 0, 1.0, 0.3), movedBuffer = new StandInBuffer();
movedBuffer.splatCount = n;
moved.build([movedBuffer], [a.boxScene], true, false);
out.movedPlain = box(moved.computeBoundingBox(false));
out.movedTransformed = box(moved.computeBoundingBox(true));
out.movedRadius = moved.maxSplatDistanceFromSceneCenter;
out.movedTransform = Array.from(moved.scenes[0].transform.elements);
console.log(JSON.stringify(out));
for (const m of [main.mesh, instant.mesh, uncalled.mesh, moved]) m.dispose();
