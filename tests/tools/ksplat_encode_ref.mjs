// tests/tools/ksplat_encode_ref.mjs — records what the REFERENCE's own .ksplat writer returns for level-0 rows:
// src/loaders/SplatBuffer.js and src/loaders/UncompressedSplatArray.js are imported in place through
// tests/tools/formats_loader.mjs.  <dir>/cases.json lists {name, file, minimumAlpha, compressionLevel, sceneCenter, blockSize,
// bucketSize}; `file` is a one-section level-0 .ksplat (gaussiansplats3d_amd.assets.write_ksplat).  Its rows are read into an
// UncompressedSplatArray entry by entry - centre, scale, the four rotation floats in slot order, the colour bytes, the SH
// floats - and SplatBuffer.generateFromUncompressedSplatArrays([rows], minimumAlpha, compressionLevel, sceneCenter, blockSize,
// bucketSize) runs on them; the returned buffer goes to <dir>/<name>.ksplat.
import fs from 'fs';
import path from 'path';
const [srcRoot, dir] = process.argv.slice(2);

const run = async () => {
  const { SplatBuffer } = await import(path.join(srcRoot, 'loaders/SplatBuffer.js'));
  const { UncompressedSplatArray } = await import(path.join(srcRoot, 'loaders/UncompressedSplatArray.js'));
  const THREE = await import('three');
  const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'));
  const manifest = {};
  for (const c of cases) {
    const b = fs.readFileSync(path.join(dir, c.file));
    const view = new DataView(b.buffer, b.byteOffset, b.byteLength);
    if (view.getUint16(20, true) !== 0 || view.getUint32(4, true) !== 1) throw new Error(`${c.name}: not a one-section level-0 file`);
    const n = view.getUint32(4096 + 4, true), degree = view.getUint16(4096 + 40, true);
    const ncomp = degree === 0 ? 0 : (degree === 1 ? 9 : 24), stride = 44 + 4 * ncomp;
    const rows = new UncompressedSplatArray(degree);
    for (let i = 0; i < n; i++) {
      const at = 4096 + 1024 + stride * i, splat = [];
      for (let k = 0; k < 10; k++) splat.push(view.getFloat32(at + 4 * k, true));
      for (let k = 0; k < 4; k++) splat.push(view.getUint8(at + 40 + k));
      for (let k = 0; k < ncomp; k++) splat.push(view.getFloat32(at + 44 + 4 * k, true));
      rows.addSplat(splat);
    }
    const sb = SplatBuffer.generateFromUncompressedSplatArrays([rows], c.minimumAlpha, c.compressionLevel,
                                                               new THREE.Vector3().fromArray(c.sceneCenter), c.blockSize, c.bucketSize);
    fs.writeFileSync(path.join(dir, `${c.name}.ksplat`), Buffer.from(sb.bufferData));
    manifest[c.name] = { splatCount: sb.getSplatCount(), bytes: sb.bufferData.byteLength };
  }
  fs.writeFileSync(path.join(dir, 'manifest.json'), JSON.stringify(manifest));
  console.log(JSON.stringify({ ok: true }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
