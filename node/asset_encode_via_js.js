// Converts a scene file to .ksplat on the device through the JS shim (test driver), with the arguments of the reference's
// util/create-ksplat.js:
//   node asset_encode_via_js.js <in file> <out.ksplat> [compression level = 0] [alpha removal threshold = 1] [scene center = "0,0,0"]
//                               [block size = 5.0] [bucket size = 256] [spherical harmonics level = 0]
// The format comes from assetFormatOf (the extension, or the file's first bytes).  Prints {format, bytes}.
'use strict';
const fs = require('fs');
const gs = require('./gsplat.js');
const argv = process.argv;
if (argv.length < 4) throw new Error('expected at least an input and an output file');
const bytes = new Uint8Array(fs.readFileSync(argv[2]));
const format = gs.assetFormatOf(argv[2], bytes);
const options = {
  compressionLevel: argv.length >= 5 ? parseInt(argv[4], 10) : undefined,
  splatAlphaRemovalThreshold: argv.length >= 6 ? parseInt(argv[5], 10) : undefined,
  sceneCenter: argv.length >= 7 ? argv[6].split(',').map(parseFloat) : undefined,
  blockSize: argv.length >= 8 ? parseFloat(argv[7]) : undefined,
  bucketSize: argv.length >= 9 ? parseInt(argv[8], 10) : undefined,
  outSphericalHarmonicsDegree: argv.length >= 10 ? parseInt(argv[9], 10) : undefined,
};
const out = gs.encodeKsplat({ bytes, format }, options);
if (!Buffer.isBuffer(out)) throw new Error('encodeKsplat did not return a Buffer');
fs.writeFileSync(argv[3], out);
console.log(JSON.stringify({ format, bytes: out.length }));
