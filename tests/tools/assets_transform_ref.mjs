// tests/tools/assets_transform_ref.mjs — records what the REFERENCE's own SplatBuffer fills return when they are handed a
// scene transform (static mode, src/splatmesh/SplatMesh.js:1872-1899): src/loaders/SplatBuffer.js and
// src/loaders/ply/INRIAV1PlyParser.js are imported in place, 'three' resolves to oracle/three_min.mjs through
// oracle/three_loader.mjs.  Per tag (ply, gen0, gen1, gen2: the files of tests/golden/assets_ref_*.npz) and per transform:
//   fillSplatCenterArray -> <tag>_<name>_centers.f32, fillSplatCovarianceArray at level 0 / 1 -> _cov.f32 / _cov.u16,
//   fillSphericalHarmonicsArray at max(1, level) -> _sh.u16 / _sh.u8, and the matrix -> <name>_matrix.f64
// for tests/tools/make_assets_transform_golden.py.
// usage: node --experimental-loader oracle/three_loader.mjs tests/tools/assets_transform_ref.mjs <reference/src> <dir> <shDegree>
//        <dir> holds in.ply and gen0.ksplat, gen1.ksplat, gen2.ksplat
import fs from 'fs';
import path from 'path';
const [srcRoot, dir, degArg] = process.argv.slice(2);
const shDegree = parseInt(degArg, 10);
const run = async () => {
  const { SplatBuffer } = await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { INRIAV1PlyParser } = await import(path.join(srcRoot, 'loaders/ply/INRIAV1PlyParser.js'));
  const THREE = await import('three');
  const bytes = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
  const dump = (name, typed) => fs.writeFileSync(path.join(dir, name), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength));

  const q1 = new THREE.Quaternion(0.3, -0.2, 0.5, 0.78).normalize(), q2 = new THREE.Quaternion(-0.6, 0.1, 0.2, 0.4).normalize();
  const compose = (p, q, s) => new THREE.Matrix4().compose(new THREE.Vector3(...p), q, new THREE.Vector3(...s));
  const transforms = {
    identity: new THREE.Matrix4(),
    rigid: compose([1.5, -2, 0.25], q1, [1, 1, 1]),
    uniform: compose([1.5, -2, 0.25], q1, [1.7, 1.7, 1.7]),
    nonuniform: compose([-0.75, 0.5, 3], q2, [0.5, 2, 1.25]),
    mirror: compose([0.25, 0, -1], q2, [-1, 1, 1]),
  };
  const manifest = { shDegree, transforms: Object.keys(transforms), buffers: {} };
  for (const [name, m] of Object.entries(transforms)) dump(`${name}_matrix.f64`, new Float64Array(m.elements));

  const buffers = { ply: INRIAV1PlyParser.parseToUncompressedSplatBuffer(bytes('in.ply'), shDegree) };
  for (const level of [0, 1, 2]) buffers[`gen${level}`] = new SplatBuffer(bytes(`gen${level}.ksplat`));
  for (const [tag, sb] of Object.entries(buffers)) {
    const n = sb.getSplatCount(), deg = Math.min(shDegree, sb.getMinSphericalHarmonicsDegree());
    const ncoef = deg === 0 ? 0 : (deg === 1 ? 9 : 24);
    const shLevel = Math.max(1, sb.compressionLevel);                          // SplatMesh.js:1064-1066
    const stats = {};
    for (const [name, m] of Object.entries(transforms)) {
      const centers = new Float32Array(3 * n), cov32 = new Float32Array(6 * n), cov16 = new Uint16Array(6 * n);
      sb.fillSplatCenterArray(centers, m, undefined, undefined, 0);
      sb.fillSplatCovarianceArray(cov32, m, undefined, undefined, 0, 0);
      sb.fillSplatCovarianceArray(cov16, m, undefined, undefined, 0, 1);
      dump(`${tag}_${name}_centers.f32`, centers); dump(`${tag}_${name}_cov.f32`, cov32); dump(`${tag}_${name}_cov.u16`, cov16);
      let finite = centers.every(Number.isFinite) && cov32.every(Number.isFinite), shChanged = null, shOnRail = null;
      const halfOverflow = cov16.some((h) => (h & 0x7fff) >= 0x7bff);
      if (ncoef) {
        const mk = () => (shLevel === 2 ? new Uint8Array(ncoef * n) : new Uint16Array(ncoef * n));
        const sh = mk(), plain = mk();
        sb.fillSphericalHarmonicsArray(sh, deg, m, undefined, undefined, 0, shLevel);
        sb.fillSphericalHarmonicsArray(plain, deg, undefined, undefined, undefined, 0, shLevel);
        dump(`${tag}_${name}_sh.${shLevel === 2 ? 'u8' : 'u16'}`, sh);
        shChanged = 0;
        for (let i = 0; i < sh.length; i++) if (sh[i] !== plain[i]) shChanged++;
        if (shLevel === 2) { shOnRail = 0; for (let i = 0; i < sh.length; i++) if (sh[i] === 0 || sh[i] === 255) shOnRail++; }
      }
      stats[name] = { finite, halfOverflow, shChanged, shOnRail };
    }
    manifest.buffers[tag] = { splatCount: n, shDegree: deg, compressionLevel: sb.compressionLevel, shLevel, ncoef, stats };
  }
  fs.writeFileSync(path.join(dir, 'transform_manifest.json'), JSON.stringify(manifest));
  console.log(JSON.stringify({ ok: true }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
