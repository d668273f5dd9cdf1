"""-m gpu: adding scenes to a live mesh and sort worker from node (node/add_scenes_via_js.mjs): meshResize / sorterResize through
the N-API addon, the sort worker's `{resize}` message followed by a `centers` message for the new range only, and
SplatMesh.addScenes of the drop-in on a static and on a dynamic mesh.  Inside node the frames and the worker's sorted list are
byte-equal to a drop-in mesh and worker built from all buffers at once; removeScenes of the added scene works on the device; a
buffer of another SH degree, a buffer still loading and a scene beyond Constants.MaxScenes take the full build."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
from gaussiansplats3d_amd import camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
SIZES = (300, 257, 443)
W = H = 64


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_add_scenes_of_the_drop_in_mesh(tmp_path, dynamic):
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    scenes = [helpers.small_scene(n, 0, 80 + k) for k, n in enumerate(SIZES)]
    cam = camera.demo_camera("garden", W, H)
    fx, fy = cam.focal()
    positions = [[0.0, 0.0, 0.0], [0.5, 0.25, 0.0], [-0.25, 0.5, 0.125]]
    job = {"scenes": [{"centers": s.centers.reshape(-1).tolist(), "cov": s.cov.reshape(-1).tolist(), "rgba": s.rgba.reshape(-1).tolist(),
                       "position": p} for s, p in zip(scenes, positions)],
           "dynamic": dynamic, "order": np.random.default_rng(9).permutation(sum(SIZES)).tolist(), "width": W, "height": H, "focal": [fx, fy],
           "matrixWorld": np.linalg.inv(np.asarray(cam.view, np.float64).reshape(4, 4).T).T.reshape(16).tolist(),
           "view": np.asarray(cam.view, np.float64).reshape(16).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(16).tolist(),
           "sortMvp": np.asarray(cam.sort_mvp(), np.float64).reshape(16).tolist()}
    (tmp_path / "in.json").write_text(json.dumps(job))
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(NODE_DIR, "add_scenes_via_js.mjs"), str(tmp_path / "in.json")],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=300)
    got = json.loads(out.strip().splitlines()[-1])
    # a 33rd scene takes the full build, which answers as a build of all 33 buffers does: the device holds 32 scene indexes
    limit = got.pop("sceneLimitError")
    assert limit is not None and "GS_MAX_SCENES" in limit, limit
    got.pop("sceneLimitFallback", None)
    assert got == {key: True for key in got}, got
    assert len(got) == 29, sorted(got)
