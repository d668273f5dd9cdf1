// Test driver: one frame through the JS shim, then a pick through node/Raycaster.mjs.  usage: node surface_via_js.mjs <in.json>
// in.json: {centers, cov, rgba, order, modelView (= viewMatrix * the mesh's model matrix), viewMatrix, proj, camPos, focal, width, height,
//           matrixWorld (the camera's), screen: [x, y]} (plain arrays)
import fs from 'fs';
import * as THREE from 'three';
import { createRequire } from 'module';
import { SplatMesh } from './SplatMesh.mjs';
import { Raycaster } from './Raycaster.mjs';
const require = createRequire(import.meta.url);
const gs = require('./gsplat.js');
const a = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const n = a.centers.length / 3;
const core = new gs.SplatMeshHIP(n, {});
core.build(new Float32Array(a.centers), new Float32Array(a.cov), new Uint8Array(a.rgba), null);
core.updateRenderIndexes(new Uint32Array(a.order), n);
core.updateUniforms({ x: a.width, y: a.height }, a.focal[0], a.focal[1], false, 1.0, 1.0);
core.setCameraMatrices(a.modelView, a.proj, a.camPos, a.viewMatrix);
const mesh = new SplatMesh();                               // the drop-in class around the device mesh (no SplatBuffers in this test)
mesh.core = core;
const r = core.render();
mesh.frame = { data: r.pixels, width: a.width, height: a.height, stats: r.stats };
const camera = { isPerspectiveCamera: true, matrixWorld: new THREE.Matrix4().fromArray(a.matrixWorld),
                 projectionMatrix: new THREE.Matrix4().fromArray(a.proj) };
core.setCameraMatrices(a.proj, a.modelView, [9, 9, 9], a.proj);   // a camera set AFTER the draw must not move the answer
const rc = new Raycaster();
rc.setFromCameraAndScreenPosition(camera, { x: a.screen[0], y: a.screen[1] }, { x: a.width, y: a.height });
const hits = [];
rc.intersectSplatMesh(mesh, hits);
rc.threshold = 0.3;
const none = rc.intersectSplatMesh(mesh, []);
console.log(JSON.stringify({ hits: hits.map((h) => ({ origin: h.origin.toArray(), normal: h.normal.toArray(), distance: h.distance,
                                                      splatIndex: h.splatIndex, pixel: h.pixel, depth: h.depth })),
                             noneAt03: none.length, direction: rc.ray.direction.toArray(), rayOrigin: rc.ray.origin.toArray() }));
core.dispose();
