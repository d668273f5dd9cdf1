"""The RENDER SEAM as a JavaScript drop-in, proven with the reference's own caller code (task 2).

node/SplatMesh.mjs (the reference's SplatMesh interface) and node/SortWorker.mjs (createSortWorker) are driven by the TEXT of
Viewer.addSplatBuffersToMesh / setupSortWorker / runSplatSort / gatherSceneNodesForSort / updateSplatMesh, cut out of the
reference's src/Viewer.js and evaluated under Node (tests/seam_via_viewer.mjs), with splat data from the reference's own PLY
parser -> SplatBuffer.  The cut text and the loader modules live in oracle/_ref/seam/ (built by `make -C oracle` from
/root/reference where it exists, git-ignored, shipped to the GPU box like the reference's WASM sorter).
CPU tier: the bundle is there, the modules load, the class has the reference's method names and arities.
GPU tier: the frame and the sorted index list the Viewer's code produces through the JS seam equal, bit for bit, what the ctypes
mirror (native PLY reader -> gs_mesh_* / gs_sorter_* / gs_tree_*) produces from the same file and camera."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "node")
BUNDLE = os.path.join(ROOT, "oracle", "_ref", "seam")
LOADER = os.path.join(ROOT, "oracle", "three_loader.mjs")
pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")


def _bundle():
    if not os.path.exists(os.path.join(BUNDLE, "viewer_cut.json")):       # build() makes it (oracle.build) where the reference is
        pytest.skip("oracle/_ref/seam is not built (__graft_entry__.build() makes it where the reference is present)")
    return BUNDLE


def _node(args, **kw):
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    return subprocess.check_output(["node", "--no-warnings", "--experimental-loader", LOADER] + args, cwd=os.path.join(ROOT, "tests"),
                                   text=True, **kw)


REFERENCE_METHODS = {   # name: Function.length in the reference (parameters before the first default), src/splatmesh/SplatMesh.js
    "build": 2, "getIntegerCenters": 2, "getFloatCenters": 2, "getSceneIndexes": 2, "getSplatCount": 0, "getMaxSplatCount": 0,
    "updateRenderIndexes": 2, "updateUniforms": 6, "fillTransformsArray": 1, "getSplatTree": 0, "fillSplatDataArrays": 7,
    "refreshGPUDataFromSplatBuffers": 1, "getDataForDistancesComputation": 2, "setSplatScale": 0, "setPointCloudModeEnabled": 1,
    "getScene": 1, "getSceneTransform": 2, "updateTransforms": 0, "setRenderer": 1, "freeIntermediateSplatData": 0,
    "getSplatDataTextures": 0, "onSplatTreeReady": 1, "dispose": 0}


def test_the_drop_in_class_has_the_reference_interface(tmp_path):
    """Loads without a GPU (nothing touches the device before build) and exposes the reference's names and arities; where the
    reference is present the arities are read from its own SplatMesh.js text."""
    js = tmp_path / "probe.mjs"
    js.write_text("import { SplatMesh } from '%s';\n"
                  "import { createSortWorker } from '%s';\n"
                  "const m = new SplatMesh(0, false, false, false, 1, true, true, false, 1024, 0, 2, 1.0, 0.3);\n"
                  "const out = { ctor: SplatMesh.length, worker: createSortWorker.length, methods: {}, statics: Object.getOwnPropertyNames(SplatMesh),"
                  " degree: m.sphericalHarmonicsDegree, matrixWorld: m.matrixWorld.elements.length, count: m.getSplatCount() };\n"
                  "for (const k of Object.getOwnPropertyNames(SplatMesh.prototype)) out.methods[k] = SplatMesh.prototype[k].length;\n"
                  "console.log(JSON.stringify(out));\n" % (os.path.join(NODE_DIR, "SplatMesh.mjs"), os.path.join(NODE_DIR, "SortWorker.mjs")))
    info = json.loads(_node([str(js)]).strip().splitlines()[-1])
    assert info["worker"] == 5 and info["degree"] == 2 and info["matrixWorld"] == 16 and info["count"] == 0
    for name, arity in REFERENCE_METHODS.items():
        assert info["methods"].get(name) == arity, (name, info["methods"].get(name), arity)
    for name in ("buildScenes", "createScene", "buildSplatIndexMaps", "getTotalMaxSplatCountForSplatBuffers", "getTotalSplatCountForScenes"):
        assert name in info["statics"]
    ref = "/root/reference/src/splatmesh/SplatMesh.js"
    if os.path.exists(ref):                                 # the table above is the reference's, not ours
        import re
        src = open(ref).read()
        for name, arity in REFERENCE_METHODS.items():
            m = re.search(r"^    %s(?: = function\(\) \{.*?return function)?\(([^)]*)\)" % re.escape(name), src, re.M | re.S)
            assert m, name
            params = [p.strip() for p in m.group(1).split(",") if p.strip()]
            n = 0
            for p_ in params:
                if "=" in p_:
                    break
                n += 1
            assert n == arity, (name, n, arity)


def test_the_seam_bundle_holds_the_viewer_text():
    cuts = json.load(open(os.path.join(_bundle(), "viewer_cut.json")))
    for key, needle in (("addSplatBuffersToMesh", "this.splatMesh.build(allSplatBuffers, allSplatBufferOptions, true, finalBuild"),
                        ("setupSortWorker", "createSortWorker(maxSplatCount, this.sharedMemoryForWorkers"),
                        ("runSplatSort", "this.sortWorker.postMessage({"), ("gatherSceneNodesForSort", "this.splatMesh.getSplatTree()"),
                        ("updateSplatMesh", "this.splatMesh.updateUniforms(renderDimensions"),
                        ("queueCentersAndSetupWorker", "'centers': buildResults.centers.buffer")):
        assert needle in cuts[key], key


def _scene_ply(n, sh_degree, seed):
    """An INRIA-v1 .ply in front of the garden camera (trainer layout: log scales, logit opacity, channel-major f_rest)."""
    from gaussiansplats3d_amd import assets, camera
    rng = np.random.default_rng(seed)
    pos, look = np.array(camera.DEMO_POSES["garden"][1]), np.array(camera.DEMO_POSES["garden"][2])
    fwd = (look - pos) / np.linalg.norm(look - pos)
    centers = (pos + fwd * rng.uniform(0.5, 9.0, size=(n, 1)) + rng.normal(size=(n, 3)) * 1.2).astype(np.float32)
    n_rest = {0: 0, 1: 9, 2: 24}[sh_degree]
    return assets.write_ply(centers, rng.normal(np.log(0.05), 0.7, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32),
                            rng.normal(0, 1.0, size=(n, 3)).astype(np.float32), rng.normal(1.0, 2.5, size=n).astype(np.float32),
                            rng.normal(0, 0.15, size=(n, n_rest)).astype(np.float32) if n_rest else None)


@pytest.mark.gpu
@pytest.mark.parametrize("final_build,shared,half", [(False, False, False), (True, False, False), (True, True, True)])
def test_viewer_text_through_the_js_seam_equals_the_ctypes_path(tmp_path, final_build, shared, half):
    from gaussiansplats3d_amd import Context, SplatMesh, SplatTree, assets, camera, create_sort_worker, util
    bundle = _bundle()
    n, deg, W, H = 20000, 2, 640, 360
    ply = _scene_ply(n, deg, seed=404)
    (tmp_path / "scene.ply").write_bytes(ply)
    cam = camera.demo_camera("garden", W, H)
    cfg = dict(width=W, height=H, shDegree=deg, fov=camera.THREE_FOV_DEG, matrixWorld=np.asarray(cam.matrix_world).tolist(),
               projection=np.asarray(cam.projection).tolist(), finalBuild=final_build, sharedMemoryForWorkers=shared,
               halfPrecisionCovariancesOnGPU=half, sceneOptions={})
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    _node([os.path.join(ROOT, "tests", "seam_via_viewer.mjs"), bundle, str(tmp_path / "scene.ply"), str(tmp_path), str(tmp_path / "cfg.json")],
          timeout=300)
    meta = json.load(open(tmp_path / "meta.json"))
    js_frame = np.fromfile(tmp_path / "frame.u8", dtype=np.uint8).reshape(H, W, 4)
    js_sorted = np.fromfile(tmp_path / "sorted.u32", dtype=np.uint32)
    assert meta["splatCount"] == n and meta["width"] == W and meta["height"] == H and js_frame[..., 3].any()
    assert meta["splatSortCount"] == meta["splatRenderCount"] == meta["renderCountHanded"] == len(js_sorted)
    assert (meta["leaves"] > 0) == final_build

    # the ctypes mirror on the same file and the numbers the Viewer's code handed over
    ctx = Context(0)
    a = assets.load(ply, spherical_harmonics_degree=deg, minimum_alpha=1, half_precision_covariances=False)
    mesh = SplatMesh(ctx, n, deg, half_precision_covariances=half)
    mesh.build(a["centers"], a["cov"], a["rgba"], a["sh_f16"])
    mesh.update_uniforms((W, H), meta["focal"][0], meta["focal"][1], False, 1.0, 1.0, model_view=meta["view"], projection=meta["proj"],
                         camera_position=meta["camPos"], view_matrix=meta["view"])
    ci = util.integer_centers(a["centers"])
    worker = create_sort_worker(ctx, n)
    worker.post_message({"centers": ci, "range": {"from": 0, "to": n - 1, "count": n}})
    mvp = np.asarray(meta["modelViewProj"], dtype=np.float64)
    if final_build:
        tree = SplatTree(ctx, 8, 1000).process_splat_mesh(a["centers"], alphas=a["rgba"][:, 3], min_alpha=1)
        assert int(tree.info().leaves) == meta["leaves"]
        r = tree.gather_scene_nodes_for_sort(cam, sort_worker=worker, to_host=False, model_view=meta["baseModelView"])
        assert r["splatRenderCount"] == meta["splatRenderCount"]
        reply = worker.sort_gathered(mvp)
        tree.dispose()
    else:
        assert meta["splatRenderCount"] == n
        reply = worker.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n}})
    np.testing.assert_array_equal(reply["sortedIndexes"], js_sorted)
    mesh.update_render_indexes(js_sorted, len(js_sorted))
    frame, stats = mesh.render()
    assert int(stats.visible_splats) == meta["visible"]
    np.testing.assert_array_equal(frame, js_frame)
    worker.terminate(); mesh.dispose(); ctx.close()
