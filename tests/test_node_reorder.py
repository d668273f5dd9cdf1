"""-m gpu: the fold of a progressive load's Morton runs through the JavaScript drop-in (node/SplatMesh.mjs, driven by
node/reorder_via_js.mjs).  One buffer is built in five update builds.  With foldRunsAtFinalBuild = true the final build leaves the
storage layout (gs_mesh_debug_read 12 through the addon's test hook) and the frame of a drop-in that built the finished buffer
once; with the property at its default the layout is the five-run one, which reorderScenes() by hand folds all the same.  The
layouts are also held to morton_ref's prediction and the frame to the Python mirror's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import morton_ref
from gaussiansplats3d_amd import Context, SplatMesh, camera

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 64
COUNTS = [300, 557, 1000, 1256, 1500]                      # splats loaded at every build; run borders inside a block and on a block edge


def test_the_final_build_folds_the_runs_of_a_progressive_load(tmp_path):
    n = COUNTS[-1]
    scene = helpers.small_scene(n, 0, seed=83)
    c, cov, rgba = scene.centers, scene.cov, scene.rgba
    cam = camera.demo_camera("garden", W, H)
    order = np.random.default_rng(12).permutation(n).astype(np.uint32)
    job = {"centers": c.reshape(-1).astype(np.float64).tolist(), "cov": cov.reshape(-1).astype(np.float64).tolist(),
           "rgba": rgba.reshape(-1).tolist(), "sceneCenter": c.mean(axis=0).astype(np.float64).tolist(), "counts": COUNTS,
           "order": order.tolist(), "width": W, "height": H, "focal": list(cam.focal(1.0)),
           "matrixWorld": np.asarray(cam.matrix_world, np.float64).reshape(-1).tolist(),
           "view": np.asarray(cam.view, np.float64).reshape(-1).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(-1).tolist()}
    (tmp_path / "in.json").write_text(json.dumps(job))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "node")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(ROOT, "node", "reorder_via_js.mjs"), str(tmp_path / "in.json"), str(tmp_path)],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=120)
    got = json.loads(out.strip().splitlines()[-1])
    whole = [[0, n]]
    assert got == {"folded": {"defaultOff": True, "skippedWhileLoading": 0, "spansAtTheEnd": whole},
                   "pieces": {"defaultOff": True, "skippedWhileLoading": 0, "spansAtTheEnd": whole},
                   "once": {"defaultOff": True, "skippedWhileLoading": None, "spansAtTheEnd": whole}}

    pos = {name: np.fromfile(tmp_path / f"{name}.pos.u32", np.uint32) for name in ("folded", "pieces", "once", "pieces_folded_by_hand")}
    one_run = morton_ref.positions(c)
    starts = [0] + COUNTS[:-1]
    five_runs = np.concatenate([morton_ref.positions(c[b:e], b) for b, e in zip(starts, COUNTS)])
    assert not np.array_equal(one_run, five_runs)          # (the pieces do not give the final order by themselves)
    assert np.array_equal(pos["once"], one_run)
    assert np.array_equal(pos["folded"], pos["once"])
    assert np.array_equal(pos["pieces"], five_runs)        # the default: every existing mesh keeps the layout it describes
    assert np.array_equal(pos["pieces_folded_by_hand"], pos["once"])

    ctx = Context(0)
    mesh = SplatMesh(ctx, n, 0)
    mesh.build(c, cov, rgba, None)
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, n)
    expect = mesh.render()[0]
    mesh.dispose()
    ctx.close()
    assert expect.any()
    for name in ("folded", "pieces", "once"):
        assert np.array_equal(np.fromfile(tmp_path / f"{name}.u8", np.uint8).reshape(H, W, 4), expect), name
