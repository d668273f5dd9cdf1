// tests/tools/formats_ref.mjs — records what the REFERENCE's own parsers and SplatBuffer fills return for .splat and
// PlayCanvas compressed PLY files: src/loaders/splat/SplatParser.js, src/loaders/ply/PlyParser.js (which dispatches to
// PlayCanvasCompressedPlyParser.js) and src/loaders/SplatBuffer.js are imported in place through tests/tools/formats_loader.mjs.
// <dir>/cases.json lists {name, file, kind, degree}:
//   kind 'splat'        SplatParser.parseToUncompressedSplatBufferSection into SplatBuffer.preallocateUncompressed(n, 0)
//   kind 'progressive'  PlayCanvasCompressedPlyParser.decodeHeader + readElementData(chunk) +
//                       parseToUncompressedSplatBufferSection (the path that loads a file without an `sh` element)
//   kind 'whole'        PlyParser.parseToUncompressedSplatBuffer(buffer, degree)
// Per case: <name>_centers.f32, _cov.f32 / _cov.u16 (levels 0 / 1), _rgba1.u8 / _rgba40.u8 (minimum alpha 1 / 40), _sh.u16
// (level 1), _scales.f32, _rotations.f32, and centres / covariances again under <dir>/matrix.f64 as _xf_*.
import fs from 'fs';
import path from 'path';
const [srcRoot, dir] = process.argv.slice(2);
const run = async () => {
  const { SplatBuffer } = await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { SplatParser } = await import(path.join(srcRoot, 'loaders/splat/SplatParser.js'));
  const { PlyParser } = await import(path.join(srcRoot, 'loaders/ply/PlyParser.js'));
  const { PlayCanvasCompressedPlyParser: PC } = await import(path.join(srcRoot, 'loaders/ply/PlayCanvasCompressedPlyParser.js'));
  const THREE = await import('three');
  const bytes = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
  const dump = (name, typed) => fs.writeFileSync(path.join(dir, name), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength));
  const matrix = new THREE.Matrix4();
  matrix.elements = Array.from(new Float64Array(bytes('matrix.f64')));
  const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'));
  const manifest = {};
  for (const c of cases) {
    const file = bytes(c.file);
    let sb;
    if (c.kind === 'splat') {
      const n = file.byteLength / SplatParser.RowSizeBytes;
      const { splatBuffer, splatBufferDataOffsetBytes } = SplatBuffer.preallocateUncompressed(n, 0);
      SplatParser.parseToUncompressedSplatBufferSection(0, n - 1, file, 0, splatBuffer.bufferData, splatBufferDataOffsetBytes);
      sb = splatBuffer;
    } else if (c.kind === 'progressive') {
      const header = PC.decodeHeader(file);
      const vertexAt = PC.readElementData(header.chunkElement, file, header.headerSizeBytes, null, null, null);
      const n = header.vertexElement.count;
      const { splatBuffer, splatBufferDataOffsetBytes } = SplatBuffer.preallocateUncompressed(n, 0);
      PC.parseToUncompressedSplatBufferSection(header.chunkElement, header.vertexElement, 0, n - 1, 0,
                                               file.slice(vertexAt, vertexAt + n * header.bytesPerSplat), splatBuffer.bufferData,
                                               splatBufferDataOffsetBytes);
      sb = splatBuffer;
    } else {
      sb = PlyParser.parseToUncompressedSplatBuffer(file, c.degree);
    }
    const n = sb.getSplatCount(), deg = sb.getMinSphericalHarmonicsDegree();
    const ncoef = deg === 0 ? 0 : (deg === 1 ? 9 : 24);
    const shLevel = Math.max(1, sb.compressionLevel);                          // SplatMesh.js:1064-1066
    for (const [tag, m] of [['', undefined], ['xf_', matrix]]) {
      const centers = new Float32Array(3 * n), cov32 = new Float32Array(6 * n), cov16 = new Uint16Array(6 * n);
      sb.fillSplatCenterArray(centers, m, undefined, undefined, 0);
      sb.fillSplatCovarianceArray(cov32, m, undefined, undefined, 0, 0);
      sb.fillSplatCovarianceArray(cov16, m, undefined, undefined, 0, 1);
      dump(`${c.name}_${tag}centers.f32`, centers); dump(`${c.name}_${tag}cov.f32`, cov32); dump(`${c.name}_${tag}cov.u16`, cov16);
      if (ncoef && !m) {
        const sh = new Uint16Array(ncoef * n);
        sb.fillSphericalHarmonicsArray(sh, deg, undefined, undefined, undefined, 0, shLevel);
        dump(`${c.name}_sh.u16`, sh);
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
