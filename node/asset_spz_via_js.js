// Opens a .spz file by name through the device decode of the JS shim and draws one frame (test driver): the format comes from
// assetFormatOf (the extension, or the gzip magic), the library inflates the file itself.
//   node asset_spz_via_js.js <file.spz> <in.bin> <out.bin>
// in.bin: uint32 {width, height, shDegree, 0}, modelView F32[16], proj F32[16], camPos F32[3], focal F32[2], modelViewProj F32[16]
// (the sort's).  out.bin: the sorted indexes U32[n], then the frame U8[4 * width * height].
'use strict';
const fs = require('fs');
const gs = require('./gsplat.js');
const [filePath, inPath, outPath] = process.argv.slice(2);
const bytes = new Uint8Array(fs.readFileSync(filePath));
const format = gs.assetFormatOf(filePath, bytes);
if (format !== gs.AssetFormat.spz) throw new Error(`assetFormatOf(${filePath}) = ${format}, not AssetFormat.spz`);
if (gs.assetFormatOf('renamed.bin', bytes) !== gs.AssetFormat.spz) throw new Error('the gzip magic alone does not answer spz');
const buf = fs.readFileSync(inPath);
const ab = buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength);
const [width, height, shDegree] = new Uint32Array(ab, 0, 4);
let off = 16;
const take = (count) => { const a = new Float32Array(ab.slice(off, off + count * 4)); off += count * 4; return a; };
const modelView = take(16), proj = take(16), camPos = take(3), focal = take(2), mvp = take(16);
const info = gs.addon.assetLoad(bytes, format, shDegree, 1, 0), n = info.splatCount;
const mesh = new gs.SplatMeshHIP(n, { sphericalHarmonicsDegree: info.shDegree, sphericalHarmonics8Bit: false });
const uploaded = mesh.buildFromAsset(bytes, format);
const worker = gs.createSortWorker(n, false, true, true, false);
worker.synchronous = true;
worker.uploadAssetCenters(bytes, format, shDegree);
worker.onmessage = (e) => {
  if (!e.data.sortDone) return;
  const order = e.data.sortedIndexes;
  mesh.updateRenderIndexes(order, n);
  mesh.updateUniforms({ x: width, y: height }, focal[0], focal[1], false, 1.0, 1.0);
  mesh.setCameraMatrices(modelView, proj, camPos);
  const { pixels } = mesh.render();
  fs.writeFileSync(outPath, Buffer.concat([Buffer.from(order.buffer, order.byteOffset, order.byteLength),
                                           Buffer.from(pixels.buffer, pixels.byteOffset, pixels.byteLength)]));
  console.log(JSON.stringify({ splatCount: n, uploaded, format, shDegree: info.shDegree }));
  worker.terminate();
  mesh.dispose();
};
worker.postMessage({ sort: { modelViewProj: mvp, splatRenderCount: n, splatSortCount: n } });
