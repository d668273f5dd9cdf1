// tests/tools/surfel_shader_dump.mjs — TEST INFRASTRUCTURE.  Asks the REFERENCE's own 2D material builder for its GLSL: imports
// <reference/src>/splatmesh/SplatMaterial2D.js in place ('three' -> oracle/three_min.mjs through oracle/three_loader.mjs) and calls
// SplatMaterial2D.build(dynamicMode, enableOptionalEffects, splatScale, pointCloudModeEnabled, maxSphericalHarmonicsDegree) for
// every permutation asked for; the vertex / fragment strings go to <outdir>/<name>.vert / .frag (scratch files of
// tests/tools/make_surfel_golden.py under oracle/_ref/, never committed).
// usage: node --experimental-loader oracle/three_loader.mjs surfel_shader_dump.mjs <reference/src> <outdir> <perms.json>
import fs from 'fs';
import path from 'path';
const [srcRoot, outDir, permsPath] = process.argv.slice(2);
const run = async () => {
  const { SplatMaterial2D } = await import(path.join(srcRoot, 'splatmesh/SplatMaterial2D.js'));
  const perms = JSON.parse(fs.readFileSync(permsPath, 'utf8'));
  for (const p of perms) {
    const m = SplatMaterial2D.build(!!p.dynamicMode, !!p.enableOptionalEffects, 1.0, false, p.maxSphericalHarmonicsDegree);
    fs.writeFileSync(path.join(outDir, p.name + '.vert'), m.vertexShader);
    fs.writeFileSync(path.join(outDir, p.name + '.frag'), m.fragmentShader);
    fs.writeFileSync(path.join(outDir, p.name + '.state.json'), JSON.stringify({ transparent: m.transparent, blending: m.blending,
      depthTest: m.depthTest, depthWrite: m.depthWrite, side: m.side }));
  }
  console.log(JSON.stringify({ ok: true, count: perms.length }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
