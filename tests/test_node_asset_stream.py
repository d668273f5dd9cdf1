"""-m gpu: a streamed file through the JavaScript drop-in (node/SplatMesh.mjs buildFromStream, driven by node/stream_via_js.mjs).
An INRIA-v1 PLY is handed over in seven appends cut inside the header, at its end and in the middle of rows; every append is an update build whose new rows go to the
mesh and the sort worker on the device.  The drop-in built that way shows the sort order and the frame of the drop-in that received
the whole file in one append - and of the Python mirror's whole-file asset; with foldRunsAtFinalBuild it also has the storage layout
of one upload.  What every append reports as ready is the model's count."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import asset_stream_cases as SC
import helpers
import test_gpu_asset_upload as U
from gaussiansplats3d_amd import Context, assets, camera

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 64
N = 1500


def test_the_drop_in_built_from_a_stream_shows_what_the_whole_file_shows(tmp_path):
    scene = helpers.small_scene(N, 0, seed=83)
    data = SC.v1_file(N, 9, 91, extra_uchar=True, centers=scene.centers)
    model = SC.Model(data, "ply", 1)
    stride = model.runs[0][2]
    ends = [model.header_at - 5, model.header_at, model.header_at + 300 * stride + 17, model.header_at + 557 * stride - 1, model.header_at + 1000 * stride,
            model.header_at + 1256 * stride + stride // 2, len(data)]
    cam = camera.demo_camera("garden", W, H)
    (tmp_path / "file.ply").write_bytes(data)
    job = {"file": str(tmp_path / "file.ply"), "format": 1, "shDegree": 1, "ends": ends,
           "modelViewProj": np.asarray(cam.sort_mvp(), np.float64).reshape(-1).tolist(), "width": W, "height": H,
           "focal": list(cam.focal(1.0)), "matrixWorld": np.asarray(cam.matrix_world, np.float64).reshape(-1).tolist(),
           "view": np.asarray(cam.view, np.float64).reshape(-1).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(-1).tolist()}
    (tmp_path / "in.json").write_text(json.dumps(job))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "node")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(ROOT, "node", "stream_via_js.mjs"), str(tmp_path / "in.json"), str(tmp_path)],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=120)
    got = json.loads(out.strip().splitlines()[-1])

    ready = [model.at(e)[1] for e in ends[:-1]] + [N]
    # a cut inside the header; the header alone; a cut inside row 300; one byte short of row 556
    assert ready[:4] == [0, 0, 300, 556], ready
    for name in ("pieces", "folded"):
        assert [a["ready"] for a in got[name]["appends"]] == ready, name
        # (before the header is in there is nothing to build; with the header and no row yet the build is one of no splats)
        assert [a["count"] for a in got[name]["appends"][:2]] == [None, 0], name
        starts = [a["from"] for a in got[name]["appends"] if a["count"]]
        assert starts == [0, 300, 556, 1000, 1256], "every append with new rows uploaded exactly [last ready, ready)"
    for name in ("pieces", "folded", "whole"):
        assert (got[name]["splatCount"], got[name]["complete"], got[name]["uploaded"]) == (N, 1, N), name
        assert got[name]["treeLeaves"], "the final build built the splat tree from the completed stream"

    order = {name: np.fromfile(tmp_path / f"{name}.order.u32", np.uint32) for name in got}
    frame = {name: np.fromfile(tmp_path / f"{name}.u8", np.uint8).reshape(H, W, 4) for name in got}
    pos = {name: np.fromfile(tmp_path / f"{name}.pos.u32", np.uint32) for name in got}
    assert np.array_equal(pos["folded"], pos["whole"]), "foldRunsAtFinalBuild leaves the layout of one upload"
    assert not np.array_equal(pos["pieces"], pos["whole"])
    for name in ("pieces", "folded"):
        assert np.array_equal(order[name], order["whole"]) and np.array_equal(frame[name], frame["whole"]), name

    ctx = Context(0)                                         # ... and the Python mirror's whole-file asset
    asset = assets.SplatAsset(data, "ply", 1)
    pair = U.Pair(ctx, asset, N, False, True, False, 1, cam)
    try:
        pair.host(0, 0, N)
        seen = pair.observe()
        assert seen["frame"].any()
        assert np.array_equal(order["whole"], seen["order"]) and np.array_equal(frame["whole"], seen["frame"])
    finally:
        pair.close()
        asset.close()
        ctx.close()
