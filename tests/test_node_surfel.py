"""-m gpu: SplatRenderMode.TwoD through the JavaScript drop-in (node/SplatMesh.mjs, driven by node/surfel_via_js.mjs).  The drop-in
accepts the mode, pulls scales and rotations through fillSplatDataArrays with the reference's scaleOverride.z = 1
(/root/reference/src/splatmesh/SplatMesh.js:1856-1863), packs them as updateScaleRotationsPaddedData does and draws one frame case
of tests/surfel_cases.py: the frame and the vertex-stage records equal the Python mirror's bit for bit.  getSplatScaleAndRotation
reports scale z = 0 (:1991)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import surfel_cases
from gaussiansplats3d_amd import Context, SplatMesh

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_drop_in_draws_a_surfel_frame_case_as_the_python_mirror_does(tmp_path):
    case, order, _ = surfel_cases.frame_case("mixed_branches")
    cam, n = case["camera"], case["centers"].shape[0]
    f64 = lambda x: np.asarray(x, np.float64).reshape(-1).tolist()      # noqa: E731
    job = {"centers": f64(case["centers"]), "scales": f64(case["scales"]), "rotations": f64(case["rotations"]),
           "rgba": case["rgba"].reshape(-1).tolist(), "sceneCenter": f64(case["centers"].mean(axis=0)), "order": order.tolist(),
           "width": cam.width, "height": cam.height, "focal": list(cam.focal(1.0)), "matrixWorld": f64(cam.matrix_world),
           "view": f64(cam.view), "proj": f64(cam.projection)}
    (tmp_path / "in.json").write_text(json.dumps(job))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "node")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(ROOT, "node", "surfel_via_js.mjs"), str(tmp_path / "in.json"), str(tmp_path)],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=120)
    got = json.loads(out.strip().splitlines()[-1])
    assert got["refusesOther"] and got["uploadedScaleZ"] == 1 and got["scaleZ"] == 0
    assert got["scaleX"] == pytest.approx(float(case["scales"][0, 0]))

    ctx = Context(0)
    mesh = SplatMesh(ctx, n, 0, render_mode_2d=True)
    mesh.build(case["centers"], None, case["rgba"], scales=case["scales"], rotations=case["rotations"])
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, n)
    expect = mesh.render()[0]
    records = mesh.debug_records_2d()[0]
    mesh.dispose()
    ctx.close()
    assert expect.any()
    assert np.array_equal(np.fromfile(tmp_path / "records.u32", np.uint32).reshape(n, 20), records)
    assert np.array_equal(np.fromfile(tmp_path / "frame.u8", np.uint8).reshape(cam.height, cam.width, 4), expect)
