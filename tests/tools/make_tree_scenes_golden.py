"""tests/tools/make_tree_scenes_golden.py — records the REFERENCE's dynamic-mode octree cull for the cases of
tests/tree_scenes_cases.py into tests/golden/tree_scenes_ref.json: one sub-tree per scene from the reference's own worker, then
Viewer.gatherSceneNodesForSort with dynamicMode: true, run under Node by tests/tools/tree_scenes_ref.mjs.  Per case the file holds
the inputs' seed, the sub-trees' leaf counts and, per pose, the base modelView (inverse(camera.matrixWorld) as the reference computes
it, fp64 bit patterns), splatRenderCount and the full index list.  Runs only where the reference's sources exist.
usage: python tests/tools/make_tree_scenes_golden.py <reference/src>"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import tree_scenes_cases as cases  # noqa: E402


def main(ref):
    golden = {}
    for name in cases.NAMES:
        case = cases.make_case(name)
        keep = cases.keep_mask(case)
        scenes = []
        for a, b in cases.scene_ranges(case):
            # SplatTree.processSplatMesh's addCentersForScene: (x, y, z, global index) of the splats the filter keeps
            ids = np.arange(a, b) if keep is None else np.arange(a, b)[keep[a:b]]
            c4 = np.zeros((len(ids), 4), np.float32)
            c4[:, :3] = case["centers"][ids]
            c4[:, 3] = ids
            scenes.append([float(v) for v in c4.reshape(-1)])
        script = cases.make_script(name)
        doc = dict(maxDepth=case["max_depth"], maxCentersPerNode=case["max_centers"], splatCount=int(case["scene_counts"].sum()),
                   scenes=scenes, transforms=[t.tolist() for t in case["transforms"]], meshWorld=case["mesh_world"].tolist(),
                   poses=[dict(matrixWorld=p["matrix_world"].tolist(), fov=p["fov"], width=p["width"], height=p["height"],
                               gatherAll=p["gather_all"]) for p in script])
        with tempfile.TemporaryDirectory() as d:
            json.dump(doc, open(os.path.join(d, "case.json"), "w"))
            subprocess.check_call(["node", "--no-warnings", os.path.join(HERE, "tree_scenes_ref.mjs"), f"{ref}/splattree/SplatTree.js",
                                   f"{ref}/Viewer.js", f"{ref}/Constants.js", os.path.join(d, "case.json"), os.path.join(d, "out.json")])
            out = json.load(open(os.path.join(d, "out.json")))
        golden[name] = dict(seed=case["seed"], splats=doc["splatCount"], subTreeLeaves=out["subTreeLeaves"],
                            poses=[dict(tag=p["tag"], **r) for p, r in zip(script, out["poses"])])
        print(name, out["subTreeLeaves"], [r["splatRenderCount"] for r in out["poses"]])
    with open(os.path.join(ROOT, "tests", "golden", "tree_scenes_ref.json"), "w") as f:
        json.dump(golden, f, separators=(",", ":"))


if __name__ == "__main__":
    main(sys.argv[1])
