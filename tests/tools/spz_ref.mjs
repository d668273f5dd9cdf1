// tests/tools/spz_ref.mjs — records what the REFERENCE's own .spz loader and SplatBuffer fills return for .spz files:
// src/loaders/spz/SpzLoader.js and src/loaders/SplatBuffer.js are imported in place through tests/tools/formats_loader.mjs.
// The loader is written for a browser; four stand-ins let it run unmodified under Node, all built on zlib.gunzipSync:
//   window.setTimeout     Util.delayedExecute
//   ReadableStream        Compression.createStream: start(controller) with enqueue / close, and pipeThrough
//   DecompressionStream   'gzip' only
//   Response              arrayBuffer() of the piped stream
// (gunzipSync accepts bytes behind the member's trailer, where a browser's DecompressionStream errors: this script cannot
// show what the reference does with such a file, and the goldens hold none.)
// <dir>/cases.json lists {name, file, degree}: SpzLoader.loadFromFileData(bytes, 1, 0, false, degree) - optimizeSplatData
// false, the file-order level-0 SplatBuffer.
// Per case: <name>_centers.f32, _cov.f32 / _cov.u16 (levels 0 / 1), _rgba1.u8 / _rgba40.u8 (minimum alpha 1 / 40), _sh.u16
// (level 1), _scales.f32, _rotations.f32, and centres, covariances and SH again under <dir>/matrix.f64 as _xf_*.
import fs from 'fs';
import path from 'path';
import zlib from 'zlib';
const [srcRoot, dir] = process.argv.slice(2);

globalThis.window = { setTimeout: (f, ms) => setTimeout(f, ms) };
globalThis.ReadableStream = class {
  constructor(source) {
    this.chunks = [];
    this.started = source.start({ enqueue: (d) => this.chunks.push(Buffer.from(d)), close: () => {} });
  }
  pipeThrough(transform) { transform.source = this; return transform; }
};
globalThis.DecompressionStream = class {
  constructor(format) { if (format !== 'gzip') throw new Error('stand-in: gzip only'); }
};
globalThis.Response = class {
  constructor(piped) { this.piped = piped; }
  async arrayBuffer() {
    await this.piped.source.started;
    const b = zlib.gunzipSync(Buffer.concat(this.piped.source.chunks));
    return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength);
  }
};

const run = async () => {
  await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { SpzLoader } = await import(path.join(srcRoot, 'loaders/spz/SpzLoader.js'));
  const THREE = await import('three');
  const bytes = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
  const dump = (name, typed) => fs.writeFileSync(path.join(dir, name), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength));
  const matrix = new THREE.Matrix4();
  matrix.elements = Array.from(new Float64Array(bytes('matrix.f64')));
  const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'));
  const manifest = {};
  for (const c of cases) {
    const sb = await SpzLoader.loadFromFileData(bytes(c.file), 1, 0, false, c.degree);
    const n = sb.getSplatCount(), deg = sb.getMinSphericalHarmonicsDegree();
    const ncoef = deg === 0 ? 0 : (deg === 1 ? 9 : 24);
    const shLevel = Math.max(1, sb.compressionLevel);                          // SplatMesh.js:1064-1066
    for (const [tag, m] of [['', undefined], ['xf_', matrix]]) {
      const centers = new Float32Array(3 * n), cov32 = new Float32Array(6 * n), cov16 = new Uint16Array(6 * n);
      sb.fillSplatCenterArray(centers, m, undefined, undefined, 0);
      sb.fillSplatCovarianceArray(cov32, m, undefined, undefined, 0, 0);
      sb.fillSplatCovarianceArray(cov16, m, undefined, undefined, 0, 1);
      dump(`${c.name}_${tag}centers.f32`, centers); dump(`${c.name}_${tag}cov.f32`, cov32); dump(`${c.name}_${tag}cov.u16`, cov16);
      if (ncoef) {
        const sh = new Uint16Array(ncoef * n);
        sb.fillSphericalHarmonicsArray(sh, deg, m, undefined, undefined, 0, shLevel);
        dump(`${c.name}_${tag}sh.u16`, sh);
      }
    }
    for (const alpha of [1, 40]) {
      const rgba = new Uint8Array(4 * n);
      sb.fillSplatColorArray(rgba, alpha, undefined, undefined, 0);
      dump(`${c.name}_rgba${alpha}.u8`, rgba);
    }
    const scales = new Float32Array(3 * n), rotations = new Float32Array(4 * n);
    sb.fillSplatScaleRotationArray(scales, rotations, undefined, undefined, undefined, 0, 0);
    dump(`${c.name}_scales.f32`, scales); dump(`${c.name}_rotations.f32`, rotations);
    manifest[c.name] = { splatCount: n, shDegree: deg, ncoef, compressionLevel: sb.compressionLevel, shLevel };
  }
  fs.writeFileSync(path.join(dir, 'manifest.json'), JSON.stringify(manifest));
  console.log(JSON.stringify({ ok: true }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
