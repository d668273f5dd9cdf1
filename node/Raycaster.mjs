// Raycaster.mjs — picking for the drop-in SplatMesh, with the two public methods the reference's Raycaster is used through
// (src/raycaster/Raycaster.js: setFromCameraAndScreenPosition, intersectSplatMesh), over the engine's surface pass.
//
//     import { Raycaster } from '<this repo>/node/Raycaster.mjs';          // was './raycaster/Raycaster.js'
//
// NOT the reference's test: that one intersects the ray with a sphere per splat through the octree, ignores opacity and returns
// every sphere the ray touches, nearest first.  Here `intersectSplatMesh` asks the rasteriser itself where the surface of the LAST
// DRAWN FRAME is under the pixel (SplatMesh.surfaceAt -> gs_mesh_surface): the first splat of the pixel's near -> far list after
// which the transmittance has fallen to `threshold` (0.5: the median depth).  At most ONE hit; opacity, the fragment rule and the
// destination's depth test count.  No parity with the reference's hits is claimed.  The Viewer consumes outHits[0].origin
// (src/Viewer.js:559-568, 1780-1792), which is what this provides - a world-space point.
import * as THREE from 'three';
import { createRequire } from 'module';
const require = createRequire(import.meta.url);
const { multiply4, invert4 } = require('./gsplat.js');

export class Raycaster {
  // threshold: the transmittance at which a pixel's walk stops (0 < threshold < 1)
  constructor({ threshold = 0.5 } = {}) {
    this.threshold = threshold;
    this.ray = { origin: new THREE.Vector3(), direction: new THREE.Vector3(0, 0, -1) };    // world space, set by the method below
    this.pick = null;                                       // the pointer as a fraction of the frame, y up
  }

  // screenPosition: pixels from the TOP-left corner, as pointer events report them; the frame's rows run bottom-up, so y is flipped
  // (as Raycaster.js:18-19 does).  Keeps the pixel for intersectSplatMesh and the world-space ray through it for the hit's fields.
  setFromCameraAndScreenPosition(camera, screenPosition, screenDimensions) {
    const u = screenPosition.x / screenDimensions.x, v = 1 - screenPosition.y / screenDimensions.y;
    const view = camera.matrixWorldInverse ? camera.matrixWorldInverse.elements : invert4(camera.matrixWorld.elements);
    const back = invert4(multiply4(camera.projectionMatrix.elements, view));                 // clip space -> world
    const world = (z) => {
      const c = [2 * u - 1, 2 * v - 1, z, 1];
      const p = [0, 1, 2, 3].map((r) => back[r] * c[0] + back[4 + r] * c[1] + back[8 + r] * c[2] + back[12 + r] * c[3]);
      return new THREE.Vector3(p[0] / p[3], p[1] / p[3], p[2] / p[3]);
    };
    // the ray runs from the pixel's point on the near plane to its point on the far plane; a perspective ray starts at the eye
    const near = world(-1), far = world(1);
    if (camera.isOrthographicCamera) this.ray.origin.copy(near);
    else if (camera.isPerspectiveCamera) this.ray.origin.set(camera.matrixWorld.elements[12], camera.matrixWorld.elements[13], camera.matrixWorld.elements[14]);
    else throw new Error('Raycaster (HIP): the camera is neither perspective nor orthographic');
    this.ray.direction.copy(far).sub(near).normalize();
    this.pick = { u, v };
  }

  // pushes at most one hit of the last drawn frame: a plain object {origin (world-space THREE.Vector3), normal (the reversed ray
  // direction: the pass computes no normals), distance (from the ray's origin), splatIndex} plus {pixel, depth} of the pass
  intersectSplatMesh(splatMesh, outHits = []) {
    const frame = splatMesh.frame;
    if (!this.pick || !frame) return outHits;
    const clampTo = (t, n) => Math.min(Math.max(Math.floor(t * n), 0), n - 1);
    const x = clampTo(this.pick.u, frame.width), y = clampTo(this.pick.v, frame.height);
    const found = splatMesh.surfaceAt(x, y, this.threshold);
    if (found) {
      outHits.push({ origin: found.position, normal: this.ray.direction.clone().multiplyScalar(-1),
                     distance: found.position.distanceTo(this.ray.origin), splatIndex: found.splatIndex, pixel: { x, y }, depth: found.depth });
    }
    return outHits;
  }
}
