// tests/tools/tree_scenes_ref.mjs — TEST INFRASTRUCTURE.  Runs the REFERENCE's own dynamic-mode cull: the worker body of
// src/splattree/SplatTree.js (cut out as text, fed `centers: [c0, c1, ...]`, one array per scene) builds one sub-tree per scene,
// and the text of Viewer.gatherSceneNodesForSort (src/Viewer.js:1969-2077) runs over them with a fake `this` whose splatMesh
// has dynamicMode: true and a getSceneTransform(s, out) that copies the case's matrix.  THREE is oracle/three_min.mjs.
// usage: node tree_scenes_ref.mjs <SplatTree.js> <Viewer.js> <Constants.js> <case.json> <out.json>
//   case.json: { maxDepth, maxCentersPerNode, splatCount, scenes: [[x, y, z, globalIndex, ...]], transforms: [[16]], meshWorld: [16],
//                poses: [{ matrixWorld, fov, width, height, gatherAll }] }
import fs from 'fs';
import * as THREE from '../../oracle/three_min.mjs';
const [treePath, viewerPath, constantsPath, casePath, outPath] = process.argv.slice(2);

const cut = (src, startToken, open = '{', close = '}') => {      // text from startToken to the brace that closes its block
  const start = src.indexOf(startToken);
  if (start < 0) throw new Error(startToken + ' not found');
  let i = src.indexOf(open, start), depth = 0;
  for (; i < src.length; i++) {
    if (src[i] === open) depth++;
    else if (src[i] === close) { depth--; if (depth === 0) return src.slice(start, i + 1); }
  }
  throw new Error('unbalanced ' + startToken);
};

const run = async () => {
  const { Constants } = await import(constantsPath);
  const treeSrc = fs.readFileSync(treePath, 'utf8');
  const classes = cut(treeSrc, 'class SplatTreeNode') + '\n' + cut(treeSrc, 'class SplatSubTree') + '\n' +
                  cut(treeSrc, 'function createSplatTreeWorker(self)');
  const lib = new Function('THREE', 'var processSplatTreeNode;\n' + classes + '\nreturn { SplatSubTree, createSplatTreeWorker };')(THREE);
  const fake = { posted: null, postMessage(m) { this.posted = m; }, onmessage: null };
  lib.createSplatTreeWorker(fake);
  const c = JSON.parse(fs.readFileSync(casePath, 'utf8'));
  const centers = c.scenes.map((s) => new Float32Array(s));
  fake.onmessage({ data: { process: { centers, maxDepth: c.maxDepth, maxCentersPerNode: c.maxCentersPerNode } } });
  const subTrees = fake.posted.subTrees.map((t) => lib.SplatSubTree.convertWorkerSubTree(t, null));

  const viewerSrc = fs.readFileSync(viewerPath, 'utf8');
  const field = cut(viewerSrc, 'gatherSceneNodesForSort = function()');
  const gather = new Function('THREE', 'Constants', 'return (' + field.slice(field.indexOf('function')) + ')();')(THREE, Constants);

  const f64hex = (v) => { const b = Buffer.alloc(8); b.writeDoubleLE(v); return b.toString('hex'); };
  const poses = [];
  for (const p of c.poses) {
    const viewer = {
      getRenderDimensions(v) { v.x = p.width; v.y = p.height; },
      camera: { fov: p.fov, matrixWorld: new THREE.Matrix4().fromArray(p.matrixWorld) },
      splatMesh: { getSplatTree() { return { subTrees }; }, dynamicMode: true, matrixWorld: new THREE.Matrix4().fromArray(c.meshWorld),
                   getSceneTransform(s, out) { out.fromArray(c.transforms[s]); } },
      sortWorkerIndexesToSort: new Uint32Array(c.splatCount),
    };
    const r = gather.call(viewer, !!p.gatherAll);
    const base = new THREE.Matrix4().copy(viewer.camera.matrixWorld).invert();
    poses.push({ splatRenderCount: r.splatRenderCount, indexes: Array.from(viewer.sortWorkerIndexesToSort.slice(0, r.splatRenderCount)),
                 base: base.elements.map(f64hex) });
  }
  fs.writeFileSync(outPath, JSON.stringify({ subTreeLeaves: subTrees.map((t) => t.nodesWithIndexes.length), poses }));
};
run().catch((e) => { console.error(String(e && e.stack || e)); process.exit(1); });
