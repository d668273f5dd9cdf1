"""-m gpu: meshRemove / sorterRemove through the N-API addon and the sort worker's `remove` message (node/remove_via_js.js), and
SplatMesh.removeScenes of the drop-in (node/remove_scenes_via_js.mjs) against a drop-in mesh built from the remaining buffers: the
middle one of three scenes goes.  Inside node the frame and the list equal those of a fresh mesh / worker that only ever saw the
two scenes that stay; here the frame is held to the Python mirror's fresh mesh and the list to the CPU sort oracle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import oracle
from gaussiansplats3d_amd import Context, SplatMesh, camera, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
SIZES = (300, 257, 443)
W = H = 64


def test_remove_through_the_addon_and_the_worker_message(tmp_path):
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    scenes = [helpers.small_scene(n, 0, 70 + k) for k, n in enumerate(SIZES)]
    centers, cov, rgba = (np.concatenate([getattr(s, name) for s in scenes]) for name in ("centers", "cov", "rgba"))
    left = SIZES[0] + SIZES[2]
    order = np.random.default_rng(6).permutation(left).astype(np.uint32)
    cam = camera.demo_camera("garden", W, H)
    fx, fy = cam.focal()
    mvp = np.asarray(cam.sort_mvp(), np.float64).astype(np.float32)
    parts = [np.array(SIZES + (W, H, 0, 0, 0), np.uint32), centers.astype(np.float32), cov.astype(np.float32), rgba, order,
             util.integer_centers(centers), np.asarray(cam.model_view(), np.float64).astype(np.float32),
             np.asarray(cam.projection, np.float64).astype(np.float32), np.asarray(cam.position, np.float32), np.array([fx, fy], np.float32), mvp]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())
    res = subprocess.run(["node", "remove_via_js.js", inp, outp], cwd=NODE_DIR, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1]) == {"meshEqual": True, "sorterEqual": True}
    raw = np.fromfile(outp, dtype=np.uint8)
    frame, got_list = raw[:W * H * 4].reshape(H, W, 4), raw[W * H * 4:].view(np.uint32)
    keep = np.r_[0:SIZES[0], SIZES[0] + SIZES[1]:sum(SIZES)]
    want = oracle.sort_indexes(np.arange(left, dtype=np.uint32), util.integer_centers(centers[keep]), cam.sort_mvp())
    assert np.array_equal(got_list, want)
    ctx = Context(0)
    mesh = SplatMesh(ctx, sum(SIZES), 0)
    mesh.build(scenes[0].centers, scenes[0].cov, scenes[0].rgba, None)
    mesh.build(scenes[2].centers, scenes[2].cov, scenes[2].rgba, None, start=SIZES[0])
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, left)
    expect = mesh.render()[0]
    mesh.dispose()
    ctx.close()
    assert frame.any() and np.array_equal(frame, expect)


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_remove_scenes_of_the_drop_in_mesh(tmp_path, dynamic):
    """Same frame and the same list handed to updateRenderIndexes as a drop-in mesh built from the two remaining buffers; the
    worker's `remove` message waits behind an asynchronous sort in flight; a mesh that cannot be edited is built afresh."""
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    scenes = [helpers.small_scene(n, 0, 80 + k) for k, n in enumerate(SIZES)]
    cam = camera.demo_camera("garden", W, H)
    fx, fy = cam.focal()
    positions = [[0.0, 0.0, 0.0], [0.5, 0.25, 0.0], [-0.25, 0.5, 0.125]]
    left = SIZES[0] + SIZES[2]
    job = {"scenes": [{"centers": s.centers.reshape(-1).tolist(), "cov": s.cov.reshape(-1).tolist(), "rgba": s.rgba.reshape(-1).tolist(),
                       "position": p} for s, p in zip(scenes, positions)],
           "dynamic": dynamic, "order": np.random.default_rng(9).permutation(left).tolist(), "width": W, "height": H, "focal": [fx, fy],
           "matrixWorld": np.linalg.inv(np.asarray(cam.view, np.float64).reshape(4, 4).T).T.reshape(16).tolist(),
           "view": np.asarray(cam.view, np.float64).reshape(16).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(16).tolist(),
           "sortMvp": np.asarray(cam.sort_mvp(), np.float64).reshape(16).tolist()}
    (tmp_path / "in.json").write_text(json.dumps(job))
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(NODE_DIR, "remove_scenes_via_js.mjs"), str(tmp_path / "in.json")],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=300)
    got = json.loads(out.strip().splitlines()[-1])
    assert got.pop("ranges") == [[SIZES[0], SIZES[1]]] and got.pop("sceneRemap") == [0, 0, 1]
    assert got.pop("fallbackEdited") is False
    assert got == {key: True for key in got} and len(got) == 13, got
