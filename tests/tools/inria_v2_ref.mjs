// tests/tools/inria_v2_ref.mjs — records what the REFERENCE's own INRIA-v2 parser and SplatBuffer fills return for ONE codebook PLY:
// src/loaders/ply/INRIAV2PlyParser.js and src/loaders/SplatBuffer.js are imported in place through tests/tools/formats_loader.mjs.
// The reference has no file-order path for this format (PlyParser.parseToUncompressedSplatBuffer throws "not implemented"), so the
// file-order level-0 buffer is put together from its own pieces: INRIAV2PlyParser.parseToUncompressedSplatArray(file, degree) parses
// every row (file order, nothing dropped), and SplatBuffer.writeSplatDataToSectionBuffer(splat, ..., 0, degree) stores splat i as
// row i of SplatBuffer.preallocateUncompressed(n, degree) - what the INRIA-v1 and .spz file-order paths do with their rows.
// One process per case: parseToUncompressedSplat keeps its raw row in a closure across calls, so a file that lacks a field would
// see the previous file's last row.
// Dumps what formats_ref.mjs dumps: <name>_centers.f32, _cov.f32 / _cov.u16, _rgba1.u8 / _rgba40.u8, _sh.u16, _scales.f32,
// _rotations.f32, centres / covariances under <dir>/matrix.f64 as _xf_*, and <name>.json.
// usage: node --experimental-loader tests/tools/formats_loader.mjs tests/tools/inria_v2_ref.mjs <reference/src> <dir> <name> <file> <degree>
import fs from 'fs';
import path from 'path';
const [srcRoot, dir, name, fileName, degreeArg] = process.argv.slice(2);
const run = async () => {
  const { SplatBuffer } = await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { INRIAV2PlyParser } = await import(path.join(srcRoot, 'loaders/ply/INRIAV2PlyParser.js'));
  const THREE = await import('three');
  const bytes = (f) => { const b = fs.readFileSync(path.join(dir, f)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
  const dump = (f, typed) => fs.writeFileSync(path.join(dir, f), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength));
  const matrix = new THREE.Matrix4();
  matrix.elements = Array.from(new Float64Array(bytes('matrix.f64')));
  const file = bytes(fileName);
  const header = INRIAV2PlyParser.decodeHeaderFromBuffer(file);
  const vertex = header.sectionHeaders.find((s) => s.sectionName !== 'codebook_centers');
  const degree = Math.min(parseInt(degreeArg), vertex.sphericalHarmonicsDegree);
  const splats = INRIAV2PlyParser.parseToUncompressedSplatArray(file, degree).splats;
  const n = splats.length;
  const { splatBuffer: sb, splatBufferDataOffsetBytes: base } = SplatBuffer.preallocateUncompressed(n, degree);
  const bytesPerSplat = SplatBuffer.CompressionLevels[0].SphericalHarmonicsDegrees[degree].BytesPerSplat;
  for (let i = 0; i < n; i++) SplatBuffer.writeSplatDataToSectionBuffer(splats[i], sb.bufferData, base + i * bytesPerSplat, 0, degree);
  const deg = sb.getMinSphericalHarmonicsDegree();
  const ncoef = deg === 0 ? 0 : (deg === 1 ? 9 : 24);
  const shLevel = Math.max(1, sb.compressionLevel);                            // SplatMesh.js:1064-1066
  for (const [tag, m] of [['', undefined], ['xf_', matrix]]) {
    const centers = new Float32Array(3 * n), cov32 = new Float32Array(6 * n), cov16 = new Uint16Array(6 * n);
    sb.fillSplatCenterArray(centers, m, undefined, undefined, 0);
    sb.fillSplatCovarianceArray(cov32, m, undefined, undefined, 0, 0);
    sb.fillSplatCovarianceArray(cov16, m, undefined, undefined, 0, 1);
    dump(`${name}_${tag}centers.f32`, centers); dump(`${name}_${tag}cov.f32`, cov32); dump(`${name}_${tag}cov.u16`, cov16);
    if (ncoef && !m) {
      const sh = new Uint16Array(ncoef * n);
      sb.fillSphericalHarmonicsArray(sh, deg, undefined, undefined, undefined, 0, shLevel);
      dump(`${name}_sh.u16`, sh);
    }
  }
  for (const alpha of [1, 40]) {
    const rgba = new Uint8Array(4 * n);
    sb.fillSplatColorArray(rgba, alpha, undefined, undefined, 0);
    dump(`${name}_rgba${alpha}.u8`, rgba);
  }
  const scales = new Float32Array(3 * n), rotations = new Float32Array(4 * n);
  sb.fillSplatScaleRotationArray(scales, rotations, undefined, undefined, undefined, 0, 0);
  dump(`${name}_scales.f32`, scales); dump(`${name}_rotations.f32`, rotations);
  fs.writeFileSync(path.join(dir, `${name}.json`),
                   JSON.stringify({ splatCount: n, shDegree: deg, ncoef, compressionLevel: sb.compressionLevel, shLevel }));
  console.log(JSON.stringify({ ok: true }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
