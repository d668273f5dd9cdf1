// tests/gpu_sort_via_viewer.mjs — the Viewer's own runSplatSort text (cut from /root/reference/src/Viewer.js into
// oracle/_ref/seam/viewer_cut.json, as tests/seam_via_viewer.mjs uses it) with `gpuAcceleratedSort: true`, against the engine's
// drop-ins: SplatMesh.computeDistancesOnGPU(mvp, sortWorkerPrecomputedDistances) runs the distance pass on the device, the sort
// worker sorts those distances (`usePrecomputedDistances`), and no `centers` message is ever posted (Viewer.js:1124-1136).
// Outputs (outDir): sorted.u32 (the list handed to updateRenderIndexes), distances.bin (what the worker received for the last
// sort), indexes.u32 (that sort's indexesToSort, splatRenderCount entries), centers.bin (the shim's getIntegerCenters / getFloatCenters, padFour), meta.json.
// usage: node --experimental-loader ../oracle/three_loader.mjs gpu_sort_via_viewer.mjs <bundle> <in.ply> <outDir> <config.json>
import fs from 'fs';
import path from 'path';
import { pathToFileURL, fileURLToPath } from 'url';
import * as THREE from 'three';
const [bundleDir, plyPath, outDir, cfgPath] = process.argv.slice(2);
const here = path.dirname(fileURLToPath(import.meta.url));
const imp = (p) => import(pathToFileURL(p).href);

const run = async () => {
  const cfg = JSON.parse(fs.readFileSync(cfgPath, 'utf8'));
  const { INRIAV1PlyParser } = await imp(path.join(bundleDir, 'src/loaders/ply/INRIAV1PlyParser.js'));
  const { Constants } = await imp(path.join(bundleDir, 'src/Constants.js'));
  const { LogLevel } = await imp(path.join(bundleDir, 'src/LogLevel.js'));
  const { SplatMesh } = await imp(path.join(here, '../node/SplatMesh.mjs'));
  const { createSortWorker } = await imp(path.join(here, '../node/SortWorker.mjs'));
  const cuts = JSON.parse(fs.readFileSync(path.join(bundleDir, 'viewer_cut.json'), 'utf8'));

  const free = { THREE, Constants, LogLevel, createSortWorker, MIN_SPLAT_COUNT_TO_SHOW_SPLAT_TREE_LOADING_SPINNER: 100000 };
  const names = Object.keys(free), values = names.map((k) => free[k]);
  const field = (text) => new Function(...names, 'return (' + text.slice(text.indexOf('function')) + ')();')(...values);   // `x = function() {...}()`
  const method = (text) => new Function(...names, 'return (function ' + text + ');')(...values);                             // `x(args) {...}`

  const buf = fs.readFileSync(plyPath);
  const ply = buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength);
  const splatBuffer = INRIAV1PlyParser.parseToUncompressedSplatBuffer(ply, cfg.shDegree);

  const camera = { fov: cfg.fov, isOrthographicCamera: false, zoom: 1, position: new THREE.Vector3(), quaternion: new THREE.Quaternion(),
                   matrixWorld: new THREE.Matrix4().fromArray(cfg.matrixWorld), projectionMatrix: new THREE.Matrix4().fromArray(cfg.projection) };
  camera.matrixWorldInverse = new THREE.Matrix4().copy(camera.matrixWorld).invert();
  camera.matrixWorld.decompose(camera.position, camera.quaternion, new THREE.Vector3());

  const viewer = {
    // the options the Viewer constructor would hold (src/Viewer.js:60-250)
    sharedMemoryForWorkers: !!cfg.sharedMemoryForWorkers, enableSIMDInSort: true, integerBasedSort: !!cfg.integer, splatSortDistanceMapPrecision: 16,
    gpuAcceleratedSort: true, logLevel: LogLevel.None, devicePixelRatio: 1, focalAdjustment: 1.0, sceneRevealMode: 2, freeIntermediateSplatData: false,
    initialized: true, sortRunning: false, preSortMessages: [], sortWorker: null, runAfterNextSort: [], splatRenderCount: 0, splatSortCount: 0,
    camera, perspectiveCamera: null, renderer: null, loadingSpinner: { addTask() { return 1; }, removeTask() {}, setMinimized() {} },
    splatMesh: new SplatMesh(0, false, false, !!cfg.halfPrecisionCovariancesOnGPU, 1, true, !!cfg.integer, !!cfg.antialiased, 1024, LogLevel.None,
                             cfg.shDegree, 1.0, 0.3),
    isDisposingOrDisposed() { return false; },
    getRenderDimensions(out) { out.x = cfg.width; out.y = cfg.height; },
    adjustForWebXRStereo() {}, forceRenderNextFrame() {}, disposeSortWorker() {},
  };
  viewer.addSplatBuffersToMesh = field(cuts.addSplatBuffersToMesh);
  viewer.setupSortWorker = method(cuts.setupSortWorker);
  viewer.runSplatSort = field(cuts.runSplatSort);
  viewer.gatherSceneNodesForSort = field(cuts.gatherSceneNodesForSort);
  viewer.updateSplatMesh = field(cuts.updateSplatMesh);
  const queueAndSetup = new Function(...names, 'return (function(splatBuffers, splatBufferOptions, finalBuild, showLoadingUIForSplatTreeBuild, ' +
    'replaceExisting, preserveVisibleRegion) { ' + cuts.queueCentersAndSetupWorker + '; return sortWorkerSetupPromise; });')(...values);
  // renderer.render(splatMesh, camera) (src/Viewer.js:1616): three calls every object's onBeforeRender
  viewer.renderer = { render(object, cam) { return object.onBeforeRender(this, null, cam); } };

  const treeReady = new Promise((resolve) => (cfg.finalBuild ? viewer.splatMesh.onSplatTreeReady(resolve) : resolve()));
  await queueAndSetup.call(viewer, [splatBuffer], [cfg.sceneOptions || {}], !!cfg.finalBuild, false, false, true);
  await treeReady;
  let handed = null;
  const realUpdate = viewer.splatMesh.updateRenderIndexes.bind(viewer.splatMesh);
  viewer.splatMesh.updateRenderIndexes = (indexes, count) => { handed = { indexes: Uint32Array.from(indexes.subarray(0, count)), count }; realUpdate(indexes, count); };
  // what the reference's code hands to the two seams: recorded so that the ctypes mirror can be driven with the same numbers
  const posted = [];
  const realPost = viewer.sortWorker.postMessage.bind(viewer.sortWorker);
  const received = [];
  const Distances = cfg.integer ? Int32Array : Float32Array;
  viewer.sortWorker.postMessage = (m) => {
    if (m.sort) {
      posted.push(Array.from(m.sort.modelViewProj));
      // what the worker reads: its shared buffer, or the array the message carries
      const d = viewer.sharedMemoryForWorkers ? new Distances(viewer.sortWorker.precomputedDistancesBuffer) : m.sort.precomputedDistances;
      const list = viewer.sharedMemoryForWorkers ? viewer.sortWorkerIndexesToSort : m.sort.indexesToSort;
      received.push({ distances: Distances.from(d), sortCount: m.sort.splatSortCount, use: m.sort.usePrecomputedDistances,
                      indexes: Uint32Array.from(list.subarray(0, m.sort.splatRenderCount)), centersPosted: false });
    }
    if (m.centers) received.push({ centersPosted: true });
    realPost(m);
  };
  let sorts = 0;
  for (;;) {                                               // the partial-sort queue: run until a sort of the whole list has landed
    await viewer.runSplatSort.call(viewer, sorts === 0, !!cfg.forceSortAll);
    await new Promise((r) => setImmediate(r));
    if (!viewer.sortPromise) break;
    await viewer.sortPromise;
    sorts++;
    if (viewer.splatSortCount >= viewer.splatRenderCount || sorts > 8) break;
  }
  const n = viewer.splatMesh.getSplatCount();
  const finalTree = viewer.splatMesh.getSplatTree();
  const last = received.filter((r) => !r.centersPosted).pop();
  const centers = viewer.splatMesh.getDataForDistancesComputation(0, n - 1).centers;
  fs.writeFileSync(path.join(outDir, 'sorted.u32'), Buffer.from(handed.indexes.buffer));
  fs.writeFileSync(path.join(outDir, 'distances.bin'), Buffer.from(last.distances.buffer, 0, 4 * n));
  fs.writeFileSync(path.join(outDir, 'indexes.u32'), Buffer.from(last.indexes.buffer));
  fs.writeFileSync(path.join(outDir, 'centers.bin'), Buffer.from(centers.buffer, centers.byteOffset, centers.byteLength));
  fs.writeFileSync(path.join(outDir, 'meta.json'), JSON.stringify({
    splatCount: n, sorts, splatRenderCount: viewer.splatRenderCount, splatSortCount: viewer.splatSortCount,
    renderCountHanded: handed.count, lastSortCount: last.sortCount, usePrecomputedDistances: last.use,
    centersPosted: received.some((r) => r.centersPosted), leaves: finalTree ? finalTree.subTrees[0].nodesWithIndexes.length : 0,
    modelViewProj: posted[posted.length - 1] }));
  if (viewer.sortWorker) viewer.sortWorker.terminate();
  await viewer.splatMesh.dispose();
  console.log(JSON.stringify({ ok: true, sorts, splatRenderCount: viewer.splatRenderCount }));
};
run().catch((e) => { console.error(e); process.exit(1); });
