// SplatMesh.mjs — drop-in for the reference's SplatMesh (/root/reference/src/splatmesh/SplatMesh.js) over the MI355X engine.
//
// Same constructor arguments, same `build(splatBuffers, sceneOptions, keepSceneTransforms, finalBuild, ...)`, same
// getIntegerCenters / getSplatCount / getMaxSplatCount / updateRenderIndexes / updateUniforms / fillTransformsArray /
// getSplatTree / setSplatScale / updateVisibleRegionFadeDistance / computeBoundingBox ..., so that the Viewer's own code - addSplatBuffersToMesh (src/Viewer.js:1189-1228),
// setupSortWorker (:1235-1300), runSplatSort (:1833-1964), gatherSceneNodesForSort (:1969-2077), updateSplatMesh
// (:651-677) and the draw `renderer.render(splatMesh, camera)` (:1616) - runs against it UNCHANGED
// (tests/test_node_seam.py executes exactly that text).  Splat data reaches the device through the SplatBuffers' own
// fillSplat*Array methods, as SplatMesh.fillSplatDataArrays (:1853-1902) does; nothing here parses files.
//
// Integration = two imports (INTEGRATION.md):
//     import { SplatMesh } from '<this repo>/node/SplatMesh.mjs';          // was './splatmesh/SplatMesh.js'
//     import { createSortWorker } from '<this repo>/node/SortWorker.mjs';  // was './worker/SortWorker.js'
// The Viewer option `gpuAcceleratedSort: true` works too: computeDistancesOnGPU runs the reference's transform-feedback distance
// pass (SplatMesh.js:1701-1814, shader :1449-1490) as a HIP kernel over the device mesh and copies the distances into the array
// the Viewer hands it (the worker's SharedArrayBuffer view or its own typed array), as getBufferSubData does there.
//
// `three` is the same peer dependency the reference imports (in this repo's tests it resolves to oracle/three_min.mjs).
// The frame lands in `this.frame` = {data: Uint8Array RGBA8 (row 0 = bottom, like gl.readPixels), width, height}; a host
// renderer shows it as a DataTexture on a full-screen quad (onBeforeRender is three's per-object hook, called by
// renderer.render).
import * as THREE from 'three';
import { createRequire } from 'module';
const require = createRequire(import.meta.url);
const { SplatMeshHIP: HipMeshCore, addon, assetAppend, Constants } = require('./gsplat.js');
import { VisibleRegion, SceneRevealMode } from './VisibleRegion.mjs';

export const SplatRenderMode = { ThreeD: 0, TwoD: 1 };
export { SceneRevealMode };

// SplatScene (src/splatmesh/SplatScene.js) without the Object3D base: the transform is compose(position, quaternion, scale)
class HipSplatScene {
  constructor(splatBuffer, position = new THREE.Vector3(), quaternion = new THREE.Quaternion(), scale = new THREE.Vector3(1, 1, 1),
              minimumAlpha = 1, opacity = 1.0, visible = true) {
    this.splatBuffer = splatBuffer;
    this.position = new THREE.Vector3().copy(position);
    this.quaternion = new THREE.Quaternion().copy(quaternion);
    this.scale = new THREE.Vector3().copy(scale);
    this.transform = new THREE.Matrix4();
    this.matrix = new THREE.Matrix4();
    this.minimumAlpha = minimumAlpha;
    this.opacity = opacity;
    this.visible = visible;
  }
  copyTransformData(other) {
    this.position.copy(other.position); this.quaternion.copy(other.quaternion); this.scale.copy(other.scale);
    this.transform.copy(other.transform);
  }
  updateTransform() {                                       // :28-36 (a scene has no parent here: matrixWorld == matrix)
    this.matrix.compose(this.position, this.quaternion, this.scale);
    this.transform.copy(this.matrix);
  }
}

// The splat-buffer face of a streamed asset (gsplat.js assetStreamOpen) for buildFromStream: the counts and header values build()
// asks a reference SplatBuffer for.  Its rows never exist on the host while it loads - the mesh and the sort worker take them from
// the stream on the device; the two fills the splat tree of the final build reads come from gs_asset_fill of the completed stream.
export class StreamedSplatBuffer {
  constructor(stream) { this.assetStream = stream; this._filled = null; }
  getSplatCount() { return this.assetStream.info.splatsReady; }
  getMaxSplatCount() { return this.assetStream.info.splatCount; }
  getMinSphericalHarmonicsDegree() { return this.assetStream.info.shDegree; }
  get compressionLevel() { return this.assetStream.info.compressionLevel; }
  get sceneCenter() { return new THREE.Vector3().fromArray(this.assetStream.info.sceneCenter); }
  get minSphericalHarmonicsCoeff() { return this.assetStream.info.shMin; }
  get maxSphericalHarmonicsCoeff() { return this.assetStream.info.shMax; }
  _fill() {
    if (!this.assetStream.info.complete) throw new Error('StreamedSplatBuffer: the host fills need the complete stream');
    return this._filled || (this._filled = addon.assetLoad(this.assetStream.handle, 0, 0, 0, 0));
  }
  fillSplatCenterArray(out, transform, from = 0, to = this.getSplatCount() - 1, dest = 0) {     // SplatBuffer.js:332-345
    const c = this._fill().centers, v = new THREE.Vector3();
    for (let i = from; i <= to; i++) {
      v.set(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
      if (transform) v.applyMatrix4(transform);
      out[3 * (i - from + dest)] = v.x; out[3 * (i - from + dest) + 1] = v.y; out[3 * (i - from + dest) + 2] = v.z;
    }
  }
  fillSplatColorArray(out, minimumAlpha, from = 0, to = this.getSplatCount() - 1, dest = 0) {    // :551-575
    const c = this._fill().rgba;
    for (let i = from; i <= to; i++) {
      const o = 4 * (i - from + dest);
      out[o] = c[4 * i]; out[o + 1] = c[4 * i + 1]; out[o + 2] = c[4 * i + 2]; out[o + 3] = c[4 * i + 3] >= minimumAlpha ? c[4 * i + 3] : 0;
    }
  }
}

export class SplatMesh {
  // Same positional arguments as the reference's constructor (src/splatmesh/SplatMesh.js:34-40); the Viewer's text reads the
  // public fields by these names.
  constructor(...args) {
    const names = ['splatRenderMode', 'dynamicMode', 'enableOptionalEffects', 'halfPrecisionCovariancesOnGPU', 'devicePixelRatio',
                   'enableDistancesComputationOnGPU', 'integerBasedDistancesComputation', 'antialiased', 'maxScreenSpaceSplatSize',
                   'logLevel', 'sphericalHarmonicsDegree', 'sceneFadeInRateMultiplier', 'kernel2DSize'];
    const defaults = [SplatRenderMode.ThreeD, false, false, false, 1, true, false, false, 1024, 0, 0, 1.0, 0.3];
    names.forEach((name, k) => { this[name] = args[k] === undefined ? defaults[k] : args[k]; });
    if (this.splatRenderMode !== SplatRenderMode.ThreeD && this.splatRenderMode !== SplatRenderMode.TwoD) throw new Error('SplatMesh (HIP): unknown splatRenderMode');
    Object.assign(this, {
      renderer: undefined, scenes: [], sceneOptions: undefined, minSphericalHarmonicsDegree: 0,
      splatTree: null, baseSplatTree: null, onSplatTreeReadyCallback: null, splatDataTextures: {},
      globalSplatIndexToLocalSplatIndexMap: [], globalSplatIndexToSceneIndexMap: [],
      lastBuildScenes: [], lastBuildSplatCount: 0, lastBuildMaxSplatCount: 0, lastBuildSceneCount: 0,
      firstRenderTime: -1, finalBuild: false, splatScale: 1.0, pointCloudModeEnabled: false,
      disposed: false, visible: false, frustumCulled: false,
      matrixWorld: new THREE.Matrix4(),                     // Object3D.matrixWorld (src/Viewer.js:1891 multiplies by it)
      core: null,                                           // the device-side mesh (gs_mesh_*)
      frame: null, shCompressionLevel: 1,
      foldRunsAtFinalBuild: false,                          // HIP-engine extra: build(..., finalBuild = true) ends a progressive load with reorderScenes()
      _region: new VisibleRegion(this.sceneFadeInRateMultiplier), _sceneCenter: new THREE.Vector3() });
    // The scene reveal's state under the reference's names (:144-149; src/Viewer.js:1585 reads visibleRegionChanging): kept by
    // node/VisibleRegion.mjs, advanced by updateVisibleRegion (every build) and updateVisibleRegionFadeDistance (every frame).
    for (const name of ['visibleRegionChanging', 'visibleRegionRadius', 'visibleRegionBufferRadius', 'visibleRegionFadeStartRadius',
                        'maxSplatDistanceFromSceneCenter']) {
      Object.defineProperty(this, name, { enumerable: true, get: () => this._region[name], set: (v) => { this._region[name] = v; } });
    }
    Object.defineProperty(this, 'calculatedSceneCenter', { enumerable: true, get: () => this._sceneCenter.fromArray(this._region.calculatedSceneCenter) });
  }

  // ---- statics, as the reference (:173-228, :1311-1341) --------------------------------------------------------------
  static buildScenes(parentObject, splatBuffers, sceneOptions) {
    const vec = (v, fallback) => new THREE.Vector3().fromArray(v || fallback);
    return splatBuffers.map((buffer, k) => {
      const o = sceneOptions[k] || {};
      return SplatMesh.createScene(buffer, vec(o.position, [0, 0, 0]), new THREE.Quaternion().fromArray(o.rotation || [0, 0, 0, 1]),
                                   vec(o.scale, [1, 1, 1]), o.splatAlphaRemovalThreshold || 1, o.opacity, o.visible);
    });
  }
  static createScene(splatBuffer, position, rotation, scale, minimumAlpha, opacity = 1.0, visible = true) {
    return new HipSplatScene(splatBuffer, position, rotation, scale, minimumAlpha, opacity, visible);
  }
  // global splat index -> (index inside its buffer, scene): every buffer owns getMaxSplatCount() consecutive global indexes
  static buildSplatIndexMaps(splatBuffers) {
    const localSplatIndexMap = [], sceneIndexMap = [];
    splatBuffers.forEach((buffer, sceneIndex) => {
      for (let local = 0, n = buffer.getMaxSplatCount(); local < n; local++) { localSplatIndexMap.push(local); sceneIndexMap.push(sceneIndex); }
    });
    return { localSplatIndexMap, sceneIndexMap };
  }
  static _sum(items, pick) { return items.reduce((n, item) => n + pick(item), 0); }
  static getTotalSplatCountForScenes(scenes) { return SplatMesh._sum(scenes, (sc) => (sc && sc.splatBuffer ? sc.splatBuffer.getSplatCount() : 0)); }
  static getTotalSplatCountForSplatBuffers(splatBuffers) { return SplatMesh._sum(splatBuffers, (b) => b.getSplatCount()); }
  static getTotalMaxSplatCountForScenes(scenes) { return SplatMesh._sum(scenes, (sc) => (sc && sc.splatBuffer ? sc.splatBuffer.getMaxSplatCount() : 0)); }
  static getTotalMaxSplatCountForSplatBuffers(splatBuffers) { return SplatMesh._sum(splatBuffers, (b) => b.getMaxSplatCount()); }

  // ---- build (:306-405) ----------------------------------------------------------------------------------------------
  build(splatBuffers, sceneOptions, keepSceneTransforms = true, finalBuild = false, onSplatTreeIndexesUpload, onSplatTreeConstruction,
        preserveVisibleRegion = true) {
    Object.assign(this, { sceneOptions, finalBuild });
    const incoming = SplatMesh.buildScenes(this, splatBuffers, sceneOptions);
    if (keepSceneTransforms) {
      const shared = Math.min(this.scenes.length, incoming.length);
      for (let k = 0; k < shared; k++) incoming[k].copyTransformData(this.getScene(k));
    }
    this.scenes = incoming;
    this.minSphericalHarmonicsDegree = splatBuffers.reduce((d, buffer) => Math.min(d, buffer.getMinSphericalHarmonicsDegree()),
                                                           Math.min(3, this.sphericalHarmonicsDegree));
    // An "update build" appends splats to the one buffer the previous build already uploaded (progressive loading); anything
    // else starts the device mesh afresh (the reference's isUpdateBuild rule, :336-352).
    const capacity = SplatMesh.getTotalMaxSplatCountForSplatBuffers(splatBuffers);
    const sameBuffers = splatBuffers.length === this.lastBuildScenes.length &&
                        splatBuffers.every((buffer, k) => buffer === this.lastBuildScenes[k].splatBuffer);
    const appendOnly = sameBuffers && this.scenes.length === 1 && this.lastBuildSceneCount === 1 && this.lastBuildMaxSplatCount === capacity;
    if (!appendOnly) {
      if (!preserveVisibleRegion) { this._region.reset(); this.firstRenderTime = -1; }       // :356-362
      Object.assign(this, { lastBuildScenes: [], lastBuildSplatCount: 0, lastBuildMaxSplatCount: 0 });
      this.disposeMeshData();
      const maps = SplatMesh.buildSplatIndexMaps(splatBuffers);
      this.globalSplatIndexToLocalSplatIndexMap = maps.localSplatIndexMap;
      this.globalSplatIndexToSceneIndexMap = maps.sceneIndexMap;
    }
    this.updateTransforms();                                // the scenes' matrices exist before the first data fill
    const uploadedUpTo = this.getSplatCount(true);
    const update = this.refreshGPUDataFromSplatBuffers(appendOnly);
    Object.assign(this, { lastBuildScenes: this.scenes.slice(), lastBuildSplatCount: uploadedUpTo,
                          lastBuildMaxSplatCount: this.getMaxSplatCount(), lastBuildSceneCount: this.scenes.length });
    if (finalBuild && this.foldRunsAtFinalBuild) this.reorderScenes();
    if (finalBuild && this.scenes.length) {
      const minAlphas = sceneOptions.map((o) => o.splatAlphaRemovalThreshold || 1);
      this.buildSplatTree(minAlphas, onSplatTreeIndexesUpload, onSplatTreeConstruction).then(() => {
        const callback = this.onSplatTreeReadyCallback;
        this.onSplatTreeReadyCallback = null;
        if (callback) callback(this.splatTree);
      });
    }
    this.visible = this.scenes.length > 0;
    return update;
  }

  // HIP-engine extra, next to the progressive path above (which it does not replace): the next piece of a streamed file
  // (gsplat.js assetStreamOpen) as an update build.  The piece is appended; the splats it made ready, [last ready, ready), go to the
  // mesh inside build() - the file's rows cross the bus and are decoded on the device (gs_mesh_upload_asset), nothing is filled
  // on the host - and to `sortWorker` as its `centers` message (gs_sorter_upload_asset_centers).  Before the header is in there
  // is nothing to build: returns null.  Else build()'s reply without `centers`.  final: the last piece; the build is the final
  // build (foldRunsAtFinalBuild and the splat tree as ever).
  buildFromStream(stream, bytes, final = false, sortWorker = null, sceneOptions = [{}]) {
    assetAppend(stream, bytes, final);
    if (!stream.info.headerReady) return null;
    if (!stream.splatBuffer) stream.splatBuffer = new StreamedSplatBuffer(stream);
    const update = this.build([stream.splatBuffer], sceneOptions, true, final);
    if (sortWorker && update.count > 0) {
      sortWorker.uploadAssetCenters(stream.handle, stream.format, stream.maxShDegree, update.from, update.from, update.count,
                                    this.dynamicMode ? new Uint32Array(update.count) : null, this._streamTransform());
    }
    return update;
  }
  // what fillSplatDataArrays hands the fills of the one scene: its transform in static mode (the identity too), none in dynamic mode
  _streamTransform() {
    if (this.dynamicMode) return null;
    const matrix = new THREE.Matrix4();
    this.getSceneTransform(0, matrix);
    return Array.from(matrix.elements);
  }

  // HIP-engine extra: a progressive load uploads every section [lastBuildSplatCount, now) as it arrives, and each upload is a
  // Morton run of its own whose 256-splat storage blocks span the scene (a trainer writes its rows in no spatial order), so the
  // vertex stage's block cull rejects nothing.  This folds every scene's getMaxSplatCount() span that holds more than one run into
  // one run on the device (gs_mesh_reorder): the layout one upload of the finished buffer would have left, no byte across the bus,
  // the numbering - and with it the sort worker's centres and the splat tree - untouched.  A scene whose buffer is still loading
  // is skipped (its span is not all uploaded).  Returns the [from, count] spans handed to the device.
  reorderScenes() {
    const spans = [];
    if (!this.core) return spans;
    let at = 0;
    for (const sc of this.scenes) {
      const n = sc.splatBuffer.getMaxSplatCount();
      if (n > 0 && sc.splatBuffer.getSplatCount() === n && at + n <= this.core.getSplatCount()) {
        try { this.core.reorder(at, n); spans.push([at, n]); } catch (e) { if (!/Morton run/.test(String(e && e.message))) throw e; }
      }
      at += n;
    }
    return spans;
  }

  // HIP-engine extra, for the body of Viewer.removeSplatScenes (src/Viewer.js:1326-1429) in place of dispose + rebuild: the scenes
  // `indexes` go away.  Host bookkeeping as a build of the remaining buffers would leave it (scenes - the same objects, so their
  // transforms stay -, sceneOptions, the two global index maps, the lastBuild* fields, the visible region through
  // updateVisibleRegion(false)); the device mesh is edited in place (gs_mesh_remove: every scene's range is its buffer's
  // getMaxSplatCount() span, as buildSplatIndexMaps numbers it) and nothing is filled or uploaded again.  Where the device cannot
  // do that - a buffer still loading (getSplatCount() < getMaxSplatCount()), or a mesh whose scenes were not uploaded one by
  // one - the device mesh is built afresh from the remaining buffers, as before.  The splat tree is disposed of either way: call
  // buildSplatTree.  Returns {edited, ranges, sceneRemap}: what the sort worker's `{remove: {ranges, sceneRemap}}` message takes
  // when edited is true (else the worker is rebuilt, as the reference does).
  removeScenes(indexes) {
    const gone = new Set(indexes);
    for (const k of gone) if (!(Number.isInteger(k) && k >= 0 && k < this.scenes.length)) throw new Error('SplatMesh::removeScenes() -> Invalid scene index.');
    const ranges = [], sceneRemap = [], survivors = [], options = [];
    let at = 0, whole = !!this.core && this.lastBuildSplatCount === this.getSplatCount(true);
    this.scenes.forEach((sc, k) => {
      const n = sc.splatBuffer.getMaxSplatCount();
      whole = whole && sc.splatBuffer.getSplatCount() === n;
      sceneRemap.push(gone.has(k) ? 0 : survivors.length);
      if (gone.has(k)) { if (n > 0) ranges.push([at, n]); } else { survivors.push(sc); options.push((this.sceneOptions || [])[k] || {}); }
      at += n;
    });
    if (!gone.size) return { edited: true, ranges, sceneRemap };
    // (a build of the remaining buffers may choose another SH degree or SH format: then the planes cannot stay)
    const degree = survivors.reduce((d, sc) => Math.min(d, sc.splatBuffer.getMinSphericalHarmonicsDegree()), Math.min(3, this.sphericalHarmonicsDegree));
    const level = survivors.length ? Math.max(1, ...survivors.map((sc) => sc.splatBuffer.compressionLevel)) : this.shCompressionLevel;
    whole = whole && degree === this.minSphericalHarmonicsDegree && level === this.shCompressionLevel;
    this.minSphericalHarmonicsDegree = degree;
    let edited = false;
    if (whole && survivors.length && ranges.length) {
      try { this.core.remove(ranges, sceneRemap); edited = true; } catch (e) { if (!/Morton run/.test(String(e && e.message))) throw e; }
    }
    this.disposeSplatTree();
    this.scenes = survivors;
    this.sceneOptions = options;
    const maps = SplatMesh.buildSplatIndexMaps(survivors.map((sc) => sc.splatBuffer));
    this.globalSplatIndexToLocalSplatIndexMap = maps.localSplatIndexMap;
    this.globalSplatIndexToSceneIndexMap = maps.sceneIndexMap;
    if (!edited) {                                          // the device mesh afresh, from the buffers that stay
      Object.assign(this, { lastBuildScenes: [], lastBuildSplatCount: 0, lastBuildMaxSplatCount: 0 });
      this.disposeMeshData();
      if (survivors.length) this.refreshDataTexturesFromSplatBuffers(false);
    }
    Object.assign(this, { lastBuildScenes: survivors.slice(), lastBuildSplatCount: this.getSplatCount(true),
                          lastBuildMaxSplatCount: this.getMaxSplatCount(), lastBuildSceneCount: survivors.length });
    this._scenesDirty = true;
    if (edited) this.updateVisibleRegion(false);            // (a refresh ends with it)
    this.visible = survivors.length > 0;
    return { edited, ranges, sceneRemap };
  }

  // HIP-engine extra, for the body of Viewer.addSplatBuffersToMesh (src/Viewer.js:1189-1226) in place of build(allSplatBuffers, ...):
  // `splatBuffers` become further scenes of a mesh that is already drawing.  Host bookkeeping as a build of all buffers leaves it
  // (the SplatScene objects that exist stay - and their transforms -, new ones are appended; sceneOptions, the two global index
  // maps, the lastBuild* fields, the visible region through updateVisibleRegion(false); the splat tree is disposed of: call
  // buildSplatTree).  The device mesh is resized to the new getMaxSplatCount() in place (gs_mesh_resize: the resident planes are
  // copied on the device) and only the new scenes are filled and uploaded - each by an upload of its own, one Morton run, so that
  // removeScenes can take it out again.  Where that cannot be - no device mesh yet, a buffer still loading, a build that would
  // choose another SH degree or SH format, more than Constants.MaxScenes scenes - the mesh is built afresh from all buffers, as
  // before.  Returns {edited, from, to, count, centers, sceneIndexes}: refreshGPUDataFromSplatBuffers' reply for the new range when
  // edited is true - post `{resize: {maxSplatCount}}` to the sort worker, then the ordinary `centers` message for that range -
  // and build()'s reply for every splat otherwise (the worker is rebuilt, as the reference does).
  addScenes(splatBuffers, sceneOptions = []) {
    const before = this.scenes.length;
    const options = Array.from({ length: before }, (_, k) => (this.sceneOptions || [])[k] || {}).concat(splatBuffers.map((_, k) => sceneOptions[k] || {}));
    const buffers = this.scenes.map((sc) => sc.splatBuffer).concat(splatBuffers);
    const degree = buffers.reduce((d, buffer) => Math.min(d, buffer.getMinSphericalHarmonicsDegree()), Math.min(3, this.sphericalHarmonicsDegree));
    const level = Math.max(1, ...buffers.map((buffer) => buffer.compressionLevel));
    const inPlace = !!this.core && before > 0 && splatBuffers.length > 0 && !this._stream() && buffers.length <= Constants.MaxScenes &&
                    buffers.every((buffer) => buffer.getSplatCount() === buffer.getMaxSplatCount()) &&
                    this.lastBuildSplatCount === this.getSplatCount(true) && degree === this.minSphericalHarmonicsDegree && level === this.shCompressionLevel;
    if (!inPlace) return Object.assign({ edited: false }, this.build(buffers, options, true, this.finalBuild));
    const from = this.getSplatCount(true);
    this.disposeSplatTree();
    const added = SplatMesh.buildScenes(this, splatBuffers, options.slice(before));
    this.scenes = this.scenes.concat(added);
    this.sceneOptions = options;
    const maps = SplatMesh.buildSplatIndexMaps(buffers);
    this.globalSplatIndexToLocalSplatIndexMap = maps.localSplatIndexMap;
    this.globalSplatIndexToSceneIndexMap = maps.sceneIndexMap;
    this.updateTransforms();                                // the new scenes' matrices exist before their data is filled
    const maxSplatCount = this.getMaxSplatCount();
    this.core.resize(maxSplatCount);
    Object.assign(this.splatDataTextures, { maxSplatCount });
    const count = this.getSplatCount(true) - from;
    const covLevel = this.getTargetCovarianceCompressionLevel(), shComponents = [0, 9, 24][this.minSphericalHarmonicsDegree];
    const xyz = new Float32Array(count * 3);                // the new range's centres, for the sort worker
    let at = 0;
    for (let k = before; k < this.scenes.length; k++) {
      const c = this.scenes[k].splatBuffer.getSplatCount();
      if (c > 0) {
        const centers = xyz.subarray(at * 3, (at + c) * 3), colors = new Uint8Array(c * 4);
        let sh = null;
        if (shComponents) sh = this.shCompressionLevel === 2 ? new Uint8Array(c * shComponents) : new Uint16Array(c * shComponents);
        const covariances = this._fillShapes(c, covLevel, centers, colors, sh, undefined, undefined, k);
        addon.meshUpload(this.core.handle, from + at, c, centers, covLevel === 1 ? null : covariances, covLevel === 1 ? covariances : null, colors,
                         sh && this.shCompressionLevel !== 2 ? sh : null);
        if (sh && this.shCompressionLevel === 2) addon.meshUploadShU8(this.core.handle, from + at, c, sh);
      }
      at += c;
    }
    this.core.splatCount = Math.max(this.core.splatCount, from + count);
    const sceneIndexes = new Uint32Array(count);
    for (let c = 0; c < count; c++) sceneIndexes[c] = this.globalSplatIndexToSceneIndexMap[from + c];
    if (count > 0) this.core.setSceneIndexes(sceneIndexes, from);   // (several scenes: the mesh holds scene indexes in every mode)
    Object.assign(this, { lastBuildScenes: this.scenes.slice(), lastBuildSplatCount: from + count,
                          lastBuildMaxSplatCount: maxSplatCount, lastBuildSceneCount: this.scenes.length });
    this._scenesDirty = true;
    this.updateVisibleRegion(false);
    this.visible = true;
    // the centres as getDataForDistancesComputation hands them over (:572-581): x1000 rounded to int32, or float; four per splat
    const centers = this.integerBasedDistancesComputation ? new Int32Array(count * 4) : new Float32Array(count * 4);
    for (let k = 0, o = 0; k < xyz.length; k += 3, o += 4) {
      if (this.integerBasedDistancesComputation) {
        centers[o] = Math.round(xyz[k] * 1000.0); centers[o + 1] = Math.round(xyz[k + 1] * 1000.0); centers[o + 2] = Math.round(xyz[k + 2] * 1000.0); centers[o + 3] = 1000;
      } else { centers[o] = xyz[k]; centers[o + 1] = xyz[k + 1]; centers[o + 2] = xyz[k + 2]; centers[o + 3] = 1.0; }
    }
    return { edited: true, from, to: from + count - 1, count, centers, sceneIndexes };
  }

  // setupDataTextures' decisions (:637-690, 1060-1090) without the textures: covariance as fp16 when asked for, SH as fp16
  // (compression level <= 1) or uint8 (level 2: kept 8-bit end to end, like the reference's sphericalHarmonics8BitMode)
  _compressionLevels() { return this.scenes.map((sc) => sc.splatBuffer.compressionLevel); }
  getMaximumSplatBufferCompressionLevel() { const l = this._compressionLevels(); return l.length ? Math.max(...l) : undefined; }
  getMinimumSplatBufferCompressionLevel() { const l = this._compressionLevels(); return l.length ? Math.min(...l) : undefined; }
  // (2D mode keeps scales and rotations in fp32 whatever halfPrecisionCovariancesOnGPU says: scaleRotationCompressionLevel 0, :666-675)
  getTargetCovarianceCompressionLevel() { return this.halfPrecisionCovariancesOnGPU && this.splatRenderMode === SplatRenderMode.ThreeD ? 1 : 0; }

  // One fillSplatDataArrays call for `count` splats and what the device stores per splat in the covariance's place: the six
  // covariance values (fp32, or half bits at covLevel 1), or - SplatRenderMode.TwoD - scale x, y, z and rotation x, y, z as
  // SplatMesh.updateScaleRotationsPaddedData packs them (:1155-1170) from the scales / rotations this pulls through
  // fillSplatDataArrays, i.e. with the reference's scaleOverride.z = 1 (:1856-1863).
  _fillShapes(count, covLevel, centers, colors, sh, srcStart, srcEnd, sceneIndex) {
    if (this.splatRenderMode !== SplatRenderMode.TwoD) {
      const covariances = covLevel === 1 ? new Uint16Array(count * 6) : new Float32Array(count * 6);
      this.fillSplatDataArrays(covariances, null, null, centers, colors, sh, undefined, covLevel, 0, this.shCompressionLevel, srcStart, srcEnd, 0, sceneIndex);
      return covariances;
    }
    const scales = new Float32Array(count * 3), rotations = new Float32Array(count * 4), packed = new Float32Array(count * 6);
    this.fillSplatDataArrays(null, scales, rotations, centers, colors, sh, undefined, 0, 0, this.shCompressionLevel, srcStart, srcEnd, 0, sceneIndex);
    for (let c = 0; c < count; c++) {
      packed[6 * c] = scales[3 * c]; packed[6 * c + 1] = scales[3 * c + 1]; packed[6 * c + 2] = scales[3 * c + 2];
      packed[6 * c + 3] = rotations[4 * c]; packed[6 * c + 4] = rotations[4 * c + 1]; packed[6 * c + 5] = rotations[4 * c + 2];
    }
    return packed;
  }
  getTargetSphericalHarmonicsCompressionLevel() { return Math.max(1, this.getMaximumSplatBufferCompressionLevel()); }

  // the stream behind the mesh's one scene (buildFromStream), or null
  _stream() { return this.scenes.length === 1 && this.scenes[0].splatBuffer.assetStream ? this.scenes[0].splatBuffer.assetStream : null; }

  // what the sort worker needs about the freshly uploaded range (the reply shape of :588-609)
  refreshGPUDataFromSplatBuffers(sinceLastBuildOnly) {
    const last = this.getSplatCount(true) - 1, first = sinceLastBuildOnly ? this.lastBuildSplatCount : 0;
    this.refreshDataTexturesFromSplatBuffers(sinceLastBuildOnly);
    if (this._stream()) return { from: first, to: last, count: last - first + 1, centers: null, sceneIndexes: this.getSceneIndexes(first, last) };
    return Object.assign({ from: first, to: last, count: last - first + 1 }, this.getDataForDistancesComputation(first, last));
  }

  // :621-635 + :900-1058: the splat buffers' own fill methods produce the arrays; they go to device planes instead of
  // padded data textures
  refreshDataTexturesFromSplatBuffers(sinceLastBuildOnly) {
    const maxSplatCount = this.getMaxSplatCount();
    const fromSplat = sinceLastBuildOnly ? this.lastBuildSplatCount : 0, toSplat = this.getSplatCount(true) - 1;
    if (!sinceLastBuildOnly || !this.core) {
      if (this.core) this.core.dispose();
      this.shCompressionLevel = this.getTargetSphericalHarmonicsCompressionLevel();
      this.core = new HipMeshCore(maxSplatCount, {
        sphericalHarmonicsDegree: this.minSphericalHarmonicsDegree, halfPrecisionCovariancesOnGPU: this.halfPrecisionCovariancesOnGPU,
        antialiased: this.antialiased, kernel2DSize: this.kernel2DSize, maxScreenSpaceSplatSize: this.maxScreenSpaceSplatSize,
        dynamicMode: this.dynamicMode, enableOptionalEffects: this.enableOptionalEffects,
        renderMode2D: this.splatRenderMode === SplatRenderMode.TwoD,
        sphericalHarmonics8Bit: this.minSphericalHarmonicsDegree > 0 && this.shCompressionLevel === 2 });
      this.core.setSplatScale(this.splatScale);
      this.core.setPointCloudModeEnabled(this.pointCloudModeEnabled);
      if (this._destination) this.setDestination(this._destination);      // a rebuilt mesh keeps the host's destination
      if (this._rop8) this.core.setRop8(true, this._rop8 === 2);          // ... and its draw mode
      this.splatDataTextures = { baseData: {}, maxSplatCount,
        covariances: { compressionLevel: this.getTargetCovarianceCompressionLevel(), size: new THREE.Vector2(maxSplatCount, 1) },
        centerColors: { size: new THREE.Vector2(maxSplatCount, 1) } };       // sizes: Viewer.js:1289-1296 only logs them
    }
    const count = toSplat - fromSplat + 1;
    if (count <= 0) { this.updateVisibleRegion(sinceLastBuildOnly); return; }
    const stream = this._stream();
    if (stream) {                                           // the rows go up as the file holds them and are decoded on the device
      // (2D mode: the device decode emits untransformed scales and rotations, so only where fillSplatDataArrays applies no
      // scene transform either - dynamicMode; a static 2D mesh takes its buffers through the host fills)
      if (this.splatRenderMode === SplatRenderMode.TwoD && !this.dynamicMode) {
        throw new Error('SplatMesh (HIP): SplatRenderMode.TwoD decodes a streamed asset on the device in dynamicMode only (no scene transform)');
      }
      addon.meshUploadAsset(this.core.handle, fromSplat, stream.handle, stream.format, stream.maxShDegree, fromSplat, count,
                            this.scenes[0].minimumAlpha, this._streamTransform());
      this.core.splatCount = Math.max(this.core.splatCount, fromSplat + count);
      if (this.dynamicMode || this.enableOptionalEffects) this.core.setSceneIndexes(new Uint32Array(count), fromSplat);
      this._scenesDirty = true;
      this.updateVisibleRegion(sinceLastBuildOnly);
      return;
    }
    const covLevel = this.getTargetCovarianceCompressionLevel();
    const centers = new Float32Array(count * 3);
    const colors = new Uint8Array(count * 4);
    const shComponents = [0, 9, 24][this.minSphericalHarmonicsDegree];
    let sh = null;
    if (shComponents) sh = this.shCompressionLevel === 2 ? new Uint8Array(count * shComponents) : new Uint16Array(count * shComponents);
    // updateBaseDataFromSplatBuffers (:900-913): source range [fromSplat, toSplat], written from 0 of these range arrays
    const covariances = this._fillShapes(count, covLevel, centers, colors, sh, sinceLastBuildOnly ? fromSplat : undefined,
                                         sinceLastBuildOnly ? toSplat : undefined, undefined);
    // A mesh of several scenes receives every scene by an upload of its own - one Morton run each, so that removeScenes can take
    // whole scenes out on the device (gs_mesh_remove refuses a border inside a run).  One scene, and a progressive load's
    // appended range, go up in one call as ever.
    const spans = [];
    if (!sinceLastBuildOnly && this.scenes.length > 1) {
      let at = 0;
      for (const sc of this.scenes) { const c = sc.splatBuffer.getSplatCount(); if (c > 0) spans.push([at, c]); at += c; }
    } else spans.push([0, count]);
    for (const [at, c] of spans) {
      const cut = (array, width) => (array ? array.subarray(at * width, (at + c) * width) : null);
      addon.meshUpload(this.core.handle, fromSplat + at, c, cut(centers, 3), covLevel === 1 ? null : cut(covariances, 6),
                       covLevel === 1 ? cut(covariances, 6) : null, cut(colors, 4), sh && this.shCompressionLevel !== 2 ? cut(sh, shComponents) : null);
    }
    if (sh && this.shCompressionLevel === 2) addon.meshUploadShU8(this.core.handle, fromSplat, count, sh);
    this.core.splatCount = Math.max(this.core.splatCount, fromSplat + count);
    if (this.scenes.length > 1 || this.dynamicMode || this.enableOptionalEffects) {
      const sceneIndexes = new Uint32Array(count);
      for (let c = 0; c < count; c++) sceneIndexes[c] = this.globalSplatIndexToSceneIndexMap[fromSplat + c];
      this.core.setSceneIndexes(sceneIndexes, fromSplat);
    }
    this._scenesDirty = true;
    this.updateVisibleRegion(sinceLastBuildOnly);           // :634
  }

  // :1172-1199.  The reference's loop over every new centre (getSplatCenter(i, c, true): the scene's transform applied in double)
  // is gs_mesh_bounds over the device mesh: a dynamic mesh stores the untransformed centres and the pass applies the scenes'
  // transforms as applyMatrix4 does (bit-equal); a static mesh stores their Float32Array rounding, which moves the radius by at
  // most 2^-24 (R + |centre|) - nothing with identity transforms.  Ends, as there, with one Default fade step; the fade uniforms
  // are only set by updateVisibleRegionFadeDistance, which the Viewer calls once per frame with its sceneRevealMode.
  updateVisibleRegion(sinceLastBuildOnly) {
    if (!this.core || !this.scenes.length) return;
    const splatCount = this.getSplatCount(true), from = sinceLastBuildOnly ? this.lastBuildSplatCount : 0;
    const transforms = this.dynamicMode ? [].concat(...this.scenes.map((sc) => sc.transform.elements)) : null;
    this._region.sceneFadeInRateMultiplier = this.sceneFadeInRateMultiplier;
    this._region.update(sinceLastBuildOnly, this.scenes.map((sc) => sc.splatBuffer.sceneCenter.toArray()), this.finalBuild,
                        (center) => (splatCount > from ? Math.sqrt(this.core.bounds(from, splatCount - from, center, transforms).maxDistSq) : 0));
  }

  // :1201-1220, once per frame (src/Viewer.js:1585-1588): advances the fade-in, then sets the vertex stage's fade uniforms
  // (GS_CAM_FADE_IN) - on while the shader's fadeInComplete is 0, off once it is 1 (always under SceneRevealMode.Instant).  A mesh
  // on which this is never called draws without a fade.
  updateVisibleRegionFadeDistance(sceneRevealMode = SceneRevealMode.Default) {
    const region = this._region;
    region.sceneFadeInRateMultiplier = this.sceneFadeInRateMultiplier;
    region.updateFadeDistance(sceneRevealMode);
    if (!this.core) return;
    if (region.shaderFadeInComplete) this.core.setFadeIn(null);
    else this.core.setFadeIn(region.calculatedSceneCenter, region.visibleRegionFadeStartRadius);
  }

  // :2066-2095.  On the device (gs_mesh_bounds) where the mesh holds the centres the reference would fill: a dynamic mesh (the
  // transforms applied by the pass when asked for), a static one whose transforms are all the identity, or a static one asked for
  // the transformed box (that is what it stores).  Otherwise through fillSplatDataArrays on the host, as the reference does.
  computeBoundingBox(applySceneTransforms = false, sceneIndex) {
    let start = 0, splatCount = this.getSplatCount();
    if (sceneIndex !== undefined && sceneIndex !== null) {
      if (sceneIndex < 0 || sceneIndex >= this.scenes.length) throw new Error('SplatMesh::computeBoundingBox() -> Invalid scene index.');
      for (let k = 0; k < sceneIndex; k++) start += this.scenes[k].splatBuffer.getSplatCount();
      splatCount = this.scenes[sceneIndex].splatBuffer.getSplatCount();
    }
    const identity = new THREE.Matrix4().elements;
    const allIdentity = this.scenes.every((sc) => sc.transform.elements.every((e, k) => e === identity[k]));
    if (this.core && (this.dynamicMode || allIdentity || applySceneTransforms)) {
      const transforms = this.dynamicMode && applySceneTransforms ? [].concat(...this.scenes.map((sc) => sc.transform.elements)) : null;
      const b = this.core.bounds(start, splatCount, [0, 0, 0], transforms);
      return new THREE.Box3(new THREE.Vector3().fromArray(b.min), new THREE.Vector3().fromArray(b.max));
    }
    const centers = new Float32Array(splatCount * 3);
    this.fillSplatDataArrays(null, null, null, centers, null, null, applySceneTransforms, undefined, undefined, undefined, undefined, undefined, 0, sceneIndex);
    const min = new THREE.Vector3(), max = new THREE.Vector3();
    for (let i = 0; i < splatCount; i++) {
      const x = centers[3 * i], y = centers[3 * i + 1], z = centers[3 * i + 2];
      if (i === 0 || x < min.x) min.x = x;
      if (i === 0 || y < min.y) min.y = y;
      if (i === 0 || z < min.z) min.z = z;
      if (i === 0 || x > max.x) max.x = x;
      if (i === 0 || y > max.y) max.y = y;
      if (i === 0 || z > max.z) max.z = z;
    }
    return new THREE.Box3(min, max);
  }

  getDataForDistancesComputation(start, end) {              // :572-581
    const centers = this.integerBasedDistancesComputation ? this.getIntegerCenters(start, end, true) : this.getFloatCenters(start, end, true);
    return { centers, sceneIndexes: this.getSceneIndexes(start, end) };
  }

  // :1853-1902, argument for argument
  fillSplatDataArrays(covariances, scales, rotations, centers, colors, sphericalHarmonics, applySceneTransform, covarianceCompressionLevel = 0,
                      scaleRotationCompressionLevel = 0, sphericalHarmonicsCompressionLevel = 1, srcStart, srcEnd, destStart = 0, sceneIndex) {
    const scaleOverride = new THREE.Vector3();                                    // :1856-1863: none in 3D, z = 1 in 2D (a surfel is flat)
    scaleOverride.x = scaleOverride.y = undefined;
    scaleOverride.z = this.splatRenderMode === SplatRenderMode.ThreeD ? undefined : 1;
    const matrix = new THREE.Matrix4();
    const oneScene = Number.isInteger(sceneIndex) && sceneIndex >= 0 && sceneIndex <= this.scenes.length;
    const firstScene = oneScene ? sceneIndex : 0, lastScene = oneScene ? sceneIndex : this.scenes.length - 1;
    if (applySceneTransform === undefined || applySceneTransform === null) applySceneTransform = !this.dynamicMode;
    if ((scales || rotations) && !(scales && rotations)) throw new Error('SplatMesh::fillSplatDataArrays() -> "scales" and "rotations" must both be valid.');
    let dest = destStart;
    for (let k = firstScene; k <= lastScene; k++) {
      const scene = this.getScene(k), buffer = scene.splatBuffer;
      let transform;                                                         // undefined = none (what the fill methods expect)
      if (applySceneTransform) { this.getSceneTransform(k, matrix); transform = matrix; }
      if (covariances) buffer.fillSplatCovarianceArray(covariances, transform, srcStart, srcEnd, dest, covarianceCompressionLevel);
      if (scales) buffer.fillSplatScaleRotationArray(scales, rotations, transform, srcStart, srcEnd, dest, scaleRotationCompressionLevel, scaleOverride);
      if (centers) buffer.fillSplatCenterArray(centers, transform, srcStart, srcEnd, dest);
      if (colors) buffer.fillSplatColorArray(colors, scene.minimumAlpha, srcStart, srcEnd, dest);
      if (sphericalHarmonics) {
        buffer.fillSphericalHarmonicsArray(sphericalHarmonics, this.minSphericalHarmonicsDegree, transform, srcStart, srcEnd, dest,
                                           sphericalHarmonicsCompressionLevel);
      }
      dest += buffer.getSplatCount();
    }
  }

  // centres of splats [start, end] as the sort worker wants them (:1912-1948): x1000 rounded to int32, or float; 3 or 4 per splat
  _centers(start, end) {
    const xyz = new Float32Array((end - start + 1) * 3);
    this.fillSplatDataArrays(null, null, null, xyz, null, null, undefined, undefined, undefined, undefined, start);
    return xyz;
  }
  getIntegerCenters(start, end, padFour = false) {
    const xyz = this._centers(start, end), stride = padFour ? 4 : 3, out = new Int32Array((xyz.length / 3) * stride);
    for (let k = 0, o = 0; k < xyz.length; k += 3, o += stride) {
      out[o] = Math.round(xyz[k] * 1000.0); out[o + 1] = Math.round(xyz[k + 1] * 1000.0); out[o + 2] = Math.round(xyz[k + 2] * 1000.0);
      if (padFour) out[o + 3] = 1000;
    }
    return out;
  }
  getFloatCenters(start, end, padFour = false) {
    const xyz = this._centers(start, end);
    if (!padFour) return xyz;
    const out = new Float32Array((xyz.length / 3) * 4);
    for (let k = 0, o = 0; k < xyz.length; k += 3, o += 4) { out[o] = xyz[k]; out[o + 1] = xyz[k + 1]; out[o + 2] = xyz[k + 2]; out[o + 3] = 1.0; }
    return out;
  }
  getSceneIndexes(start, end) {                             // (:1667-1677; written at [start, end] of the array, as there)
    const out = new Uint32Array(end - start + 1);
    for (let g = start; g <= end; g++) out[g] = this.globalSplatIndexToSceneIndexMap[g];
    return out;
  }

  // ---- counts, scenes, transforms ------------------------------------------------------------------------------------
  getSplatCount(includeSinceLastBuild = false) {
    return includeSinceLastBuild ? SplatMesh.getTotalSplatCountForScenes(this.scenes) : this.lastBuildSplatCount;
  }
  getMaxSplatCount() { return SplatMesh.getTotalMaxSplatCountForScenes(this.scenes); }
  getScene(sceneIndex) {
    const scene = this.scenes[sceneIndex];
    if (!(sceneIndex >= 0 && sceneIndex < this.scenes.length)) throw new Error('SplatMesh::getScene() -> Invalid scene index.');
    return scene;
  }
  getSceneCount() { return this.scenes.length; }
  getSceneTransform(sceneIndex, outTransform) {             // :2019-2028
    const sc = this.getScene(sceneIndex);
    sc.updateTransform(this.dynamicMode);
    outTransform.copy(sc.transform);
  }
  // :1981-1996 (with getLocalSplatParameters, :1827-1834): the scene's transform applied for a static mesh unless told otherwise;
  // scale z reads 0 in 2D mode
  getSplatScaleAndRotation(globalIndex, outScale, outRotation, applySceneTransform) {
    if (applySceneTransform === undefined || applySceneTransform === null) applySceneTransform = !this.dynamicMode;
    const sceneIndex = this.getSceneIndexForSplat(globalIndex);
    let transform = null;
    if (applySceneTransform) { transform = new THREE.Matrix4(); this.getSceneTransform(sceneIndex, transform); }
    const scaleOverride = new THREE.Vector3();
    scaleOverride.x = scaleOverride.y = scaleOverride.z = undefined;
    if (this.splatRenderMode === SplatRenderMode.TwoD) scaleOverride.z = 0;
    this.getSplatBufferForSplat(globalIndex).getSplatScaleAndRotation(this.getSplatLocalIndex(globalIndex), outScale, outRotation, transform, scaleOverride);
  }
  getSplatBufferForSplat(globalIndex) { return this.getScene(this.globalSplatIndexToSceneIndexMap[globalIndex]).splatBuffer; }
  getSceneIndexForSplat(globalIndex) { return this.globalSplatIndexToSceneIndexMap[globalIndex]; }
  getSplatLocalIndex(globalIndex) { return this.globalSplatIndexToLocalSplatIndexMap[globalIndex]; }
  updateTransforms() { this.scenes.forEach((sc) => sc.updateTransform(this.dynamicMode)); this._scenesDirty = true; }
  fillTransformsArray(array) {                              // :1683-1699: 16 floats per scene; the slots of absent scenes become NaN, as there
    const flat = new Array(array.length);
    this.scenes.forEach((sc, k) => sc.transform.elements.forEach((value, j) => { flat[16 * k + j] = value; }));
    array.set(flat);
  }
  getSplatDataTextures() { return this.splatDataTextures; }
  setRenderer(renderer) { this.renderer = renderer; }
  freeIntermediateSplatData() {}                            // nothing is kept on the host

  // :1701-1814.  Uniforms as the reference uploads them: the clip-z row of mvp (static) or of mvp * the scene's transform (dynamic,
  // one per scene), as Math.round(x * 1000) integers or as fp32.  The pass runs synchronously, so the Promise resolves with
  // `outComputedDistances` already filled (by original splat index).
  computeDistancesOnGPU(modelViewProjMatrix, outComputedDistances) {
    if (!this.core || this.core.splatCount <= 0) return Promise.resolve();
    const integer = !!this.integerBasedDistancesComputation;
    const zRow = (mat, w) => {                                // elements 2, 6, 10 (, 14) of the integer matrix: its clip-z row
      const im = SplatMesh.getIntegerMatrixArray(mat);
      return [2, 6, 10, 14].slice(0, w).map((k) => im[k]);
    };
    let uniforms, sceneCount = 1;
    if (this.dynamicMode) {
      sceneCount = this.scenes.length;
      uniforms = integer ? new Int32Array(4 * sceneCount) : new Float32Array(16 * sceneCount);
      this.scenes.forEach((scene, k) => {
        const sceneMvp = new THREE.Matrix4().multiplyMatrices(modelViewProjMatrix, scene.transform);
        if (integer) uniforms.set(zRow(sceneMvp, 4), 4 * k);               // Int32Array stores ToInt32, as gl.uniform4i does
        else uniforms.set(sceneMvp.elements, 16 * k);                      // Float32Array rounds to fp32, as gl.uniformMatrix4fv does
      });
    } else {
      uniforms = integer ? new Int32Array(zRow(modelViewProjMatrix, 3))
                         : Float32Array.from([2, 6, 10], (k) => modelViewProjMatrix.elements[k]);
    }
    this.core.computeDistances((integer ? 1 : 0) | (this.dynamicMode ? 2 : 0), uniforms, sceneCount, outComputedDistances);
    return Promise.resolve();
  }
  // :2057-2064: every element of a THREE.Matrix4 times 1000, rounded by Math.round (JS numbers, not yet int32)
  static getIntegerMatrixArray(matrix) { return Array.from(matrix.elements, (e) => Math.round(e * 1000.0)); }

  // ---- per-sort / per-frame ------------------------------------------------------------------------------------------
  updateRenderIndexes(globalIndexes, renderSplatCount) {    // :1228-1235
    if (renderSplatCount > 0 && this.firstRenderTime === -1) this.firstRenderTime = Date.now();
    if (this.core) this.core.updateRenderIndexes(globalIndexes, renderSplatCount);
  }
  updateUniforms(renderDimensions, cameraFocalLengthX, cameraFocalLengthY, orthographicMode, orthographicZoom, inverseFocalAdjustment) {   // :1248-1280
    if (this.getSplatCount() <= 0 || !this.core) return;
    this.core.updateUniforms({ x: renderDimensions.x * this.devicePixelRatio, y: renderDimensions.y * this.devicePixelRatio },
                             cameraFocalLengthX, cameraFocalLengthY, orthographicMode, orthographicZoom, inverseFocalAdjustment);
    if (this.dynamicMode || this.enableOptionalEffects) this._scenesDirty = true;
  }
  setSplatScale(splatScale = 1) { this.splatScale = splatScale; if (this.core) this.core.setSplatScale(splatScale); }
  getSplatScale() { return this.splatScale; }
  setPointCloudModeEnabled(enabled) { this.pointCloudModeEnabled = enabled; if (this.core) this.core.setPointCloudModeEnabled(enabled); }
  getPointCloudModeEnabled() { return this.pointCloudModeEnabled; }

  _uploadScenes(cameraPosition) {                           // the per-scene uniforms of updateUniforms (:1263-1276)
    const n = this.scenes.length;
    if (!(n > 1 || this.dynamicMode || this.enableOptionalEffects || (this.core.sphericalHarmonics8Bit && this.minSphericalHarmonicsDegree > 0))) return;
    const p = { sceneCount: n, transforms: new Float32Array(16 * n), invCamPos: new Float32Array(4 * n), opacity: new Float32Array(n),
                visible: new Uint32Array(n), sh8Min: new Float32Array(n), sh8Max: new Float32Array(n) };
    const inv = new THREE.Matrix4(), v = new THREE.Vector3();
    for (let i = 0; i < n; i++) {
      const scene = this.getScene(i);
      p.transforms.set(this.dynamicMode ? scene.transform.elements : new THREE.Matrix4().elements, 16 * i);
      inv.copy(scene.transform).invert();
      v.copy(cameraPosition).applyMatrix4(inv);
      p.invCamPos.set([v.x, v.y, v.z, 1], 4 * i);
      p.opacity[i] = Math.min(Math.max(scene.opacity, 0.0), 1.0);
      p.visible[i] = scene.visible ? 1 : 0;
      p.sh8Min[i] = scene.splatBuffer.minSphericalHarmonicsCoeff;
      p.sh8Max[i] = scene.splatBuffer.maxSphericalHarmonicsCoeff;
    }
    this.core.setScenes(p);
  }

  // The draw: renderer.render(splatMesh, camera) (src/Viewer.js:1616) reaches every object through onBeforeRender.
  // modelViewMatrix = camera.matrixWorldInverse * this.matrixWorld, projectionMatrix, cameraPosition: three's built-ins.
  onBeforeRender(renderer, scene, camera) { return this.renderFrame(camera); }

  // Drop-in mode (src/DropInViewer.js:34-42: the splat mesh is one object of the HOST's scene) and the Viewer's own threeScene
  // (src/Viewer.js:1610-1616: `renderer.render(this.threeScene, ...)` first, then the splat mesh with autoClear off).  The
  // reference's material is `depthTest: true, depthWrite: false` (SplatMaterial3D.js:72-73): splats behind what the other objects
  // drew are hidden, the rest blends over their colour.  A host hands that state over once per frame, after it has drawn its
  // opaque objects into a render target with a DepthTexture:
  //     renderer.readRenderTargetPixels(rt, 0, 0, w, h, colour)            -> Uint8Array RGBA8, row 0 = bottom
  //     depth: a FloatType DepthTexture copied out through a full-screen pass (or gl.readPixels(DEPTH_COMPONENT, FLOAT))
  //     splatMesh.setDestination({depth, colour, width: w, height: h, depthBits: 24})
  // and then draws `this.frame` (now the COMPLETE frame: splats over the scene) instead of blending it itself.  Pass null (or
  // nothing) to go back to splats alone over a cleared target.
  setDestination(dest) {
    this._destination = dest || null;
    if (!this.core) return;
    if (!dest) this.core.setDestination(null, null, 0, 0);
    else this.core.setDestination(dest.depth || null, dest.colour || null, dest.width, dest.height, dest.depthBits || 32);
  }
  // HIP-engine extra: draw as the browser's RGBA8 render target does (every channel rounded to 8 bits after every splat, back to
  // front: SplatMaterial3D.js:65-75 as a ROP executes it) instead of in fp32 rounded once: ~0.45 ms per 1080p frame of the garden
  // stand-in instead of 0.25; full = true walks every list to its end (~4 ms: verification).
  setRop8(enabled, full = false) {
    this._rop8 = enabled ? (full ? 2 : 1) : 0;
    if (this.core) this.core.setRop8(!!enabled, !!full);
  }
  // HIP-engine extra: the splat surface of the LAST frame at the pixel (x, y) - GL window coordinates of `this.frame`, row 0 = bottom:
  // the first splat of the pixel's near -> far list after which the transmittance has fallen to `threshold` (gs_mesh_surface: the
  // "median depth" at 0.5; opacity and the destination's depth test count, unlike the reference's ray / sphere test).  Returns
  // {splatIndex (global), depth (window depth of the splat's centre), position (THREE.Vector3, WORLD space: the pixel's centre at
  // that depth through inverse(projection * camera.matrixWorldInverse) of the frame that was drawn - this.matrixWorld is part of the
  // modelView the splats were drawn with, not of this un-projection)} or null where the pixel's splats never get there.
  // node/Raycaster.mjs wraps it in the reference Raycaster's interface.
  surfaceAt(x, y, threshold = 0.5) {
    if (!this.core || !this.frame) return null;
    const s = this.core.surfaceAt(x, y, threshold);
    return s && { splatIndex: s.splatIndex, depth: s.depth, position: new THREE.Vector3(s.position[0], s.position[1], s.position[2]) };
  }
  renderFrame(camera, out) {
    if (!this.core || this.getSplatCount() <= 0) return null;
    const view = camera.matrixWorldInverse ? camera.matrixWorldInverse : new THREE.Matrix4().copy(camera.matrixWorld).invert();
    const modelView = new THREE.Matrix4().multiplyMatrices(view, this.matrixWorld);
    const position = new THREE.Vector3().setFromMatrixPosition(camera.matrixWorld);
    this.core.setCameraMatrices(modelView.elements, camera.projectionMatrix.elements, [position.x, position.y, position.z], view.elements);
    if (this._scenesDirty) { this._uploadScenes(position); this._scenesDirty = false; }
    const r = this.core.render(out);
    this.frame = { data: r.pixels, width: this.core.cam.width, height: this.core.cam.height, stats: r.stats };
    return this.frame;
  }

  // ---- splat tree (:231-280): built by the engine (on the device), exposed in the reference's shape ---------------------
  buildSplatTree(minAlphas = [], onSplatTreeIndexesUpload, onSplatTreeConstruction) {
    this.disposeSplatTree();
    return new Promise((resolve) => {
      const total = this.getSplatCount(true), splatCount = total;
      const centers = new Float32Array(total * 3), colors = new Uint8Array(total * 4);
      // getSplatCenter / getSplatColor of every splat (:239-244): scene transforms applied as for a static mesh, alpha filter
      this.fillSplatDataArrays(null, null, null, centers, null, null, this.dynamicMode ? false : true);
      const keep = new Uint8Array(splatCount), sceneSplatCounts = new Uint32Array(this.scenes.length);
      let dest = 0;
      for (const sc of this.scenes) {
        const s = this.scenes.indexOf(sc), buffer = sc.splatBuffer, n = buffer.getSplatCount();
        sceneSplatCounts[s] = n;
        buffer.fillSplatColorArray(colors, 0, undefined, undefined, dest);
        const minAlpha = minAlphas[s] || 1;
        for (let i = 0; i < n; i++) keep[dest + i] = colors[4 * (dest + i) + 3] >= minAlpha ? 1 : 0;
        dest += n;
      }
      if (onSplatTreeIndexesUpload) onSplatTreeIndexesUpload(false);
      // maxDepth 8, 1000 per node (:236).  dynamicMode: one sub-tree per scene over the scene's untransformed centres
      // (SplatTree.js:378-386); otherwise the one tree over every (transformed) centre
      const handle = this.dynamicMode ? addon.treeCreateScenes(this.core.ctx.handle, centers, keep, sceneSplatCounts, 8, 1000) :
                                        addon.treeCreate(this.core.ctx.handle, centers, keep, splatCount, 0, 8, 1000);
      if (onSplatTreeIndexesUpload) onSplatTreeIndexesUpload(true);
      if (onSplatTreeConstruction) onSplatTreeConstruction(false);
      this.splatTree = this.baseSplatTree = new HipSplatTree(handle, this, this.dynamicMode ? this.scenes.length : 1);
      if (onSplatTreeConstruction) onSplatTreeConstruction(true);
      resolve();
    });
  }
  getSplatTree() { return this.splatTree; }
  onSplatTreeReady(callback) { this.onSplatTreeReadyCallback = callback; }
  disposeSplatTree() {
    if (this.baseSplatTree) this.baseSplatTree.dispose();
    this.splatTree = this.baseSplatTree = null;
  }
  disposeMeshData() { if (this.core) { this.core.dispose(); this.core = null; } }
  dispose() { this.disposeSplatTree(); this.disposeMeshData(); this.disposed = true; return Promise.resolve(); }
}

// SplatTree in the shape Viewer.gatherSceneNodesForSort walks (src/Viewer.js:1998-2059, src/splattree/SplatTree.js:275-318):
// subTrees[s].nodesWithIndexes[k] = {min, max, center: THREE.Vector3, data: {indexes}}.  The leaves come from gs_tree_read
// (built on the device, bit-identical to the reference's worker); `gather(...)` is the engine's own device-side gather for
// callers that skip the JS walk.  A dynamicMode mesh has one sub-tree per scene (sceneCount of them), a static one a single one.
class HipSplatTree {
  constructor(handle, splatMesh, sceneCount = 1) {
    this.handle = handle;
    this.splatMesh = splatMesh;
    this.maxDepth = 8;
    this.maxCentersPerNode = 1000;
    const t = addon.treeRead(handle), info = addon.treeInfo(handle);
    const nodes = [];
    for (let k = 0; k < t.depths.length; k++) {
      nodes.push({ min: new THREE.Vector3(t.bounds[6 * k], t.bounds[6 * k + 1], t.bounds[6 * k + 2]),
                   max: new THREE.Vector3(t.bounds[6 * k + 3], t.bounds[6 * k + 4], t.bounds[6 * k + 5]),
                   center: new THREE.Vector3(t.centers[3 * k], t.centers[3 * k + 1], t.centers[3 * k + 2]), depth: t.depths[k],
                   data: { indexes: t.indexes.subarray(t.offsets[k], t.offsets[k + 1]) }, children: [], id: k });
    }
    const first = sceneCount > 1 ? addon.treeSceneLeaves(handle, sceneCount) : [0, nodes.length];
    this.subTrees = [];
    for (let s = 0; s < sceneCount; s++) {
      this.subTrees.push({ nodesWithIndexes: nodes.slice(first[s], first[s + 1]), maxDepth: this.maxDepth, maxCentersPerNode: this.maxCentersPerNode });
    }
    this.sceneCount = sceneCount;
    this.splats = info.splats;
    this.leaves = info.allLeaves;
  }
  countLeaves() { return this.leaves; }
  visitLeaves(visitFunc) { for (const subTree of this.subTrees) for (const node of subTree.nodesWithIndexes) visitFunc(node); }
  // Viewer.gatherSceneNodesForSort (src/Viewer.js:1987-2060) on the device.  camera: {fov, matrixWorld}; renderDimensions: {x, y};
  // sorter: a device sorter's handle whose indexesToSort receives the list, or null; out: Uint32Array(splats) for a host copy,
  // or null.  Returns {splatRenderCount, shouldSortAll}.  dynamicMode: the base is inverse(camera.matrixWorld) alone (:2000) and
  // every sub-tree is tested under base x getSceneTransform(s).
  gather(camera, renderDimensions, gatherAllNodes = false, sorter = null, out = null) {
    const mesh = this.splatMesh, base = new THREE.Matrix4().copy(camera.matrixWorld).invert();
    const args = [this.handle, Float64Array.from(base.elements), camera.fov, renderDimensions.x, renderDimensions.y, gatherAllNodes ? 1 : 0];
    if (!mesh.dynamicMode) {
      args[1] = Float64Array.from(base.multiply(mesh.matrixWorld).elements);
      return { splatRenderCount: addon.treeGather(...args, sorter, out), shouldSortAll: false };
    }
    const transforms = new Float64Array(16 * this.sceneCount), matrix = new THREE.Matrix4();
    for (let s = 0; s < this.sceneCount; s++) { mesh.getSceneTransform(s, matrix); transforms.set(matrix.elements, 16 * s); }
    return { splatRenderCount: addon.treeGatherScenes(...args, transforms, sorter, out), shouldSortAll: false };
  }
  dispose() { if (this.handle) { addon.treeDestroy(this.handle); this.handle = null; } }
}

export { SplatMesh as SplatMeshHIP, HipSplatTree };
