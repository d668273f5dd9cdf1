// tests/tools/reveal_ref.mjs — records what the REFERENCE's own scene-reveal code computes, for tests/tools/make_reveal_golden.py.
// Nothing of the reference is copied: the text of the methods named below is cut out of src/splatmesh/SplatMesh.js at run time
// (brace matching from the method's name), the module's three constants are read from the same file, and the text is evaluated
// against a stub `this`:
//   updateVisibleRegion, updateVisibleRegionFadeDistance                       the state machine (:1172-1220)
//   computeBoundingBox, fillSplatDataArrays, getSceneTransform, getScene,
//   getSplatCount, static getTotalSplatCountForScenes                          the box (:2066-2095 and what it calls)
//   the `if (!preserveVisibleRegion) { ... }` block of build                   the reset (:356-362)
// The stub's getSplatCenter(i, out, true) calls the reference's own SplatBuffer.getSplatCenter (src/loaders/SplatBuffer.js, imported
// in place through tests/tools/formats_loader.mjs) of a level-0 buffer built by the reference's writer
// (preallocateUncompressed + writeSplatDataToSectionBuffer).  The stub's only own logic: the global -> (scene, local) index map, the
// material.uniforms holders, scenes = {splatBuffer, transform, updateTransform() {}} with transform = compose(position, quaternion,
// scale), and build()'s two assignments (finalBuild, lastBuildSplatCount).
// usage: node --experimental-loader tests/tools/formats_loader.mjs tests/tools/reveal_ref.mjs <reference/src> <spec.json> <out.json>
import fs from 'fs';
import path from 'path';
const [srcRoot, specFile, outFile] = process.argv.slice(2);

function cutBlock(text, openAt) {                             // the balanced {...} that starts at text[openAt]
  let depth = 0;
  for (let k = openAt; k < text.length; k++) {
    if (text[k] === '{') depth++;
    if (text[k] === '}' && --depth === 0) return text.slice(openAt, k + 1);
  }
  throw new Error('unbalanced braces');
}
function cutMethod(text, name) {                              // "(params) {body}" of the class's method `name`
  const m = new RegExp('\\n    (?:static )?' + name + '\\(').exec(text);
  if (!m) throw new Error('method not found: ' + name);
  const paren = text.indexOf('(', m.index);
  let depth = 0, close = -1;
  for (let k = paren; k < text.length; k++) {
    if (text[k] === '(') depth++;
    if (text[k] === ')' && --depth === 0) { close = k; break; }
  }
  const open = text.indexOf('{', close);
  return text.slice(paren, close + 1) + ' ' + cutBlock(text, open);
}

const run = async () => {
  const { SplatBuffer } = await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { UncompressedSplatArray } = await import(path.join(srcRoot, 'loaders/UncompressedSplatArray.js'));
  const { SceneRevealMode } = await import(path.join(srcRoot, 'SceneRevealMode.js'));
  const { SplatRenderMode } = await import(path.join(srcRoot, 'SplatRenderMode.js'));
  const THREE = await import('three');
  const text = fs.readFileSync(path.join(srcRoot, 'splatmesh/SplatMesh.js'), 'utf8');
  const constants = ['SCENE_FADEIN_RATE_FAST', 'SCENE_FADEIN_RATE_GRADUAL', 'VISIBLE_REGION_EXPANSION_DELTA'].map((name) => {
    const m = new RegExp('\\nconst ' + name + ' = ([^;]+);').exec(text);
    if (!m) throw new Error('constant not found: ' + name);
    return `const ${name} = ${m[1]};`;
  }).join('\n');
  const names = ['updateVisibleRegion', 'updateVisibleRegionFadeDistance', 'computeBoundingBox', 'fillSplatDataArrays', 'getSceneTransform',
                 'getScene', 'getSplatCount'];
  const resetAt = text.indexOf('if (!preserveVisibleRegion)');
  if (resetAt < 0) throw new Error('the reset block of build was not found');
  const resetBlock = cutBlock(text, text.indexOf('{', resetAt));
  const source = constants + '\nconst SplatMesh = { getTotalSplatCountForScenes: function' + cutMethod(text, 'getTotalSplatCountForScenes') + ' };\n' +
                 'return { ' + names.map((n) => `${n}: function${cutMethod(text, n)}`).join(',\n') + ',\nresetVisibleRegion: function() ' + resetBlock + ' };';
  const methods = new Function('THREE', 'SceneRevealMode', 'SplatRenderMode', 'performance', source)(THREE, SceneRevealMode, SplatRenderMode,
                                                                                                   { now: () => 0 });

  const levelZeroBuffer = (centers, sceneCenter) => {
    const n = centers.length / 3;
    const { splatBuffer, splatBufferDataOffsetBytes: base } = SplatBuffer.preallocateUncompressed(n, 0);
    const bytesPerSplat = SplatBuffer.CompressionLevels[0].SphericalHarmonicsDegrees[0].BytesPerSplat;
    for (let i = 0; i < n; i++) {
      const splat = UncompressedSplatArray.createSplat(0);
      splat[0] = centers[3 * i]; splat[1] = centers[3 * i + 1]; splat[2] = centers[3 * i + 2];
      SplatBuffer.writeSplatDataToSectionBuffer(splat, splatBuffer.bufferData, base + i * bytesPerSplat, 0, 0);
    }
    const f32 = new Float32Array(sceneCenter);                // a .ksplat header holds the scene centre as three floats
    splatBuffer.sceneCenter = new THREE.Vector3(f32[0], f32[1], f32[2]);
    return splatBuffer;
  };
  const makeStub = (sceneSpecs, multiplier, dynamicMode) => {
    const scenes = sceneSpecs.map((s) => {
      const transform = new THREE.Matrix4().compose(new THREE.Vector3().fromArray(s.position), new THREE.Quaternion().fromArray(s.quaternion),
                                                    new THREE.Vector3().fromArray(s.scale));
      return { splatBuffer: levelZeroBuffer(s.centers, s.sceneCenter), transform, updateTransform() {}, minimumAlpha: 1 };
    });
    const stub = Object.assign({
      scenes, dynamicMode, splatRenderMode: SplatRenderMode.ThreeD, sceneFadeInRateMultiplier: multiplier, finalBuild: false,
      lastBuildSplatCount: 0, firstRenderTime: -1, calculatedSceneCenter: new THREE.Vector3(), maxSplatDistanceFromSceneCenter: 0,
      visibleRegionBufferRadius: 0, visibleRegionRadius: 0, visibleRegionFadeStartRadius: 0, visibleRegionChanging: false,
      material: { uniformsNeedUpdate: false, uniforms: { sceneCenter: { value: new THREE.Vector3() }, visibleRegionFadeStartRadius: { value: 0 },
                  visibleRegionRadius: { value: 0 }, firstRenderTime: { value: 0 }, currentTime: { value: 0 }, fadeInComplete: { value: 0 } } },
      getSplatCenter(globalIndex, out, applySceneTransform) {
        let local = globalIndex, s = 0;
        while (local >= this.scenes[s].splatBuffer.getMaxSplatCount()) { local -= this.scenes[s].splatBuffer.getMaxSplatCount(); s++; }
        this.scenes[s].splatBuffer.getSplatCenter(local, out, applySceneTransform ? this.scenes[s].transform : undefined);
      },
    }, methods);
    return stub;
  };
  const state = (stub) => ({
    calculatedSceneCenter: stub.calculatedSceneCenter.toArray(), maxSplatDistanceFromSceneCenter: stub.maxSplatDistanceFromSceneCenter,
    visibleRegionBufferRadius: stub.visibleRegionBufferRadius, visibleRegionRadius: stub.visibleRegionRadius,
    visibleRegionFadeStartRadius: stub.visibleRegionFadeStartRadius, visibleRegionChanging: stub.visibleRegionChanging,
    shaderFadeInComplete: stub.material.uniforms.fadeInComplete.value });

  const spec = JSON.parse(fs.readFileSync(specFile, 'utf8'));
  const out = { constants: {}, bounds: [], scripts: [] };
  for (const c of spec.bounds) {
    const stub = makeStub(c.scenes, 1.0, false);
    stub.updateVisibleRegion(false);
    stub.lastBuildSplatCount = stub.getSplatCount(true);
    const box = (apply) => { const b = stub.computeBoundingBox(apply); return { min: b.min.toArray(), max: b.max.toArray() }; };
    const total = stub.getSplatCount(true), baked = new Float32Array(3 * total);
    stub.fillSplatDataArrays(null, null, null, baked, null, null, true);
    out.bounds.push({ name: c.name, transforms: stub.scenes.map((s) => Array.from(s.transform.elements)),
                      sceneCenters: stub.scenes.map((s) => s.splatBuffer.sceneCenter.toArray()),
                      calculatedSceneCenter: stub.calculatedSceneCenter.toArray(),
                      maxSplatDistanceFromSceneCenter: stub.maxSplatDistanceFromSceneCenter,
                      boxPlain: box(false), boxTransformed: box(true), bakedCenters: Array.from(baked) });
  }
  for (const sc of spec.scripts) {
    const stub = makeStub([sc.scene], sc.multiplier, false);
    const buffer = stub.scenes[0].splatBuffer;
    const events = [];
    let frame = 0;
    for (const ev of sc.events) {
      if (ev.op === 'build') {
        stub.finalBuild = ev.finalBuild;
        if (ev.reset) { stub.resetVisibleRegion(); stub.lastBuildSplatCount = 0; }
        buffer.updateLoadedCounts(1, ev.count);
        buffer.updateSectionLoadedCounts(0, ev.count);
        const from = ev.update ? stub.lastBuildSplatCount : 0;
        stub.updateVisibleRegion(ev.update);
        stub.lastBuildSplatCount = stub.getSplatCount(true);
        events.push({ op: 'build', update: ev.update, finalBuild: ev.finalBuild, reset: !!ev.reset, from, to: ev.count, state: state(stub) });
      } else {
        const samples = [];
        let flipped = stub.visibleRegionChanging === false && frame > 0;
        for (let k = 0; k < ev.count; k++, frame++) {
          const before = stub.visibleRegionChanging;
          stub.updateVisibleRegionFadeDistance(ev.mode);
          const flip = before && !stub.visibleRegionChanging && !flipped;
          if (flip) flipped = true;
          if (k < 50 || k % 25 === 0 || flip || k === ev.count - 1) samples.push({ k, flip, state: state(stub) });
        }
        events.push({ op: 'frames', mode: ev.mode, count: ev.count, samples });
      }
    }
    out.scripts.push({ name: sc.name, multiplier: sc.multiplier, sceneCenter: buffer.sceneCenter.toArray(), events });
  }
  for (const line of constants.split('\n')) { const m = /const (\w+) = (.+);/.exec(line); out.constants[m[1]] = Number(m[2]); }
  out.modes = SceneRevealMode;
  fs.writeFileSync(outFile, JSON.stringify(out));
  console.log(JSON.stringify({ ok: true }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
