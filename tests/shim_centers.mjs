// tests/shim_centers.mjs — the centres the JS drop-in's own getIntegerCenters / getFloatCenters (node/SplatMesh.mjs, padFour)
// make of fp32 centres, for checking the distance pass against what the shim would hand the reference's shader.
// usage: node --experimental-loader ../oracle/three_loader.mjs shim_centers.mjs <in.f32 (xyz per splat)> <out.i32> <out.f32>
import fs from 'fs';
import path from 'path';
import { pathToFileURL, fileURLToPath } from 'url';
const [inPath, intPath, floatPath] = process.argv.slice(2);
const here = path.dirname(fileURLToPath(import.meta.url));

const run = async () => {
  const { SplatMesh } = await import(pathToFileURL(path.join(here, '../node/SplatMesh.mjs')).href);
  const buf = fs.readFileSync(inPath);
  const xyz = new Float32Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
  const n = xyz.length / 3;
  const source = { _centers: () => xyz };                 // the splat buffers' fill, as SplatMesh._centers returns it
  const ints = SplatMesh.prototype.getIntegerCenters.call(source, 0, n - 1, true);
  const floats = SplatMesh.prototype.getFloatCenters.call(source, 0, n - 1, true);
  fs.writeFileSync(intPath, Buffer.from(ints.buffer, ints.byteOffset, ints.byteLength));
  fs.writeFileSync(floatPath, Buffer.from(floats.buffer, floats.byteOffset, floats.byteLength));
  console.log(JSON.stringify({ ok: true, n }));
};
run().catch((e) => { console.error(e); process.exit(1); });
