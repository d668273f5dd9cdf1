// tests/tools/make_distances_kat.mjs — records tests/golden/distances_kat.json: the reference's own
// SplatMesh.getIntegerMatrixArray (src/splatmesh/SplatMesh.js:2057-2064), its TEXT cut out of the reference tree and evaluated
// here, applied to matrices whose elements sit on Math.round's half-way points (+-0.0005, -0.0025, ...), on large magnitudes
// (|m * 1000| >= 2^52, where floor(t + 0.5) is not Math.round) and beyond int32; plus the Int32Array view of every result
// (ToInt32: what gl.uniform*i uploads).  tests/test_distances_uniforms.py checks the Python restatement against it.
// usage: node make_distances_kat.mjs <reference root> <out.json>
import fs from 'fs';
import path from 'path';
const [refRoot, outPath] = process.argv.slice(2);
const src = fs.readFileSync(path.join(refRoot, 'src/splatmesh/SplatMesh.js'), 'utf8');
const start = src.indexOf('static getIntegerMatrixArray(matrix)');
if (start < 0) throw new Error('getIntegerMatrixArray not found');
let i = src.indexOf('{', start), depth = 0;
for (; i < src.length; i++) {
  if (src[i] === '{') depth++;
  else if (src[i] === '}' && --depth === 0) break;
}
const text = src.slice(start, i + 1).replace(/^static\s+/, '');
const getIntegerMatrixArray = new Function('return (function ' + text + ');')();

let seed = 12345;
const rnd = () => { seed = (seed * 1103515245 + 12345) % 2147483648; return seed / 2147483648; };
const special = [0.0005, -0.0005, 0.0015, -0.0015, 0.0025, -0.0025, 0.0035, -0.0045, 1.0005, -1.0005, 2.5e-4, -2.5e-4,
                 0.0004999, -0.0005001, 0.0, -0.0, 1.0, -1.0, 2147483.647, 2147483.6475, -2147483.648, -2147483.6485,
                 4294967.296, 3e9, -3e9, 4503599627370.497, 4503599627370.4975, -4503599627370.497, 9007199254740.993,
                 1e15, -1e15, 1e300, -1e300, 5e-324, 123.4565, -123.4565];
const cases = [];
for (let k = 0; k < special.length; k += 16) {
  const e = special.slice(k, k + 16);
  while (e.length < 16) e.push(special[(k + e.length * 7) % special.length]);
  cases.push(e);
}
for (let k = 0; k < 8; k++) cases.push(Array.from({ length: 16 }, () => (rnd() - 0.5) * Math.pow(10, Math.floor(rnd() * 8) - 3)));
for (let k = 0; k < 4; k++) cases.push(Array.from({ length: 16 }, () => (Math.floor(rnd() * 20001) - 10000) / 1000 + 0.0005 * (rnd() < 0.5 ? -1 : 1)));
const out = cases.map((elements) => {
  const result = getIntegerMatrixArray({ elements });
  return { elements, round: result, int32: Array.from(new Int32Array(result)) };
});
fs.writeFileSync(outPath, JSON.stringify({ source: 'src/splatmesh/SplatMesh.js getIntegerMatrixArray', cases: out }, null, 1) + '\n');
console.log(JSON.stringify({ ok: true, cases: out.length }));
