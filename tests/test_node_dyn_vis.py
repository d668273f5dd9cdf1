"""-m gpu: the visibility-culled sort of a dynamic mesh and a dynamic-mode worker through the JS shim (node/dyn_vis_via_js.js):
setVisibilityCull(true) -> project -> postMessage({sort: {.., transforms}}) -> draw at 4097 splats under the random 30 % pattern of
dyn_vis_cases.py.  The Python rig runs the same frame first - held to the oracles by DynRig.run - and records its sorted list and
its frame in a file; the list and the frame that come out of node must equal them byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dyn_vis_cases as dyn
import vis_front_cases as cases
from gaussiansplats3d_amd import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]
N = 4097


def test_dynamic_visibility_cull_through_the_js_shim(tmp_path):
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    ctx = Context(0)
    T = cases.device_T()
    rig = dyn.DynRig(ctx, N, T, layout="runs", mode="int")
    try:
        P = cases.pattern("rand30", N, T)
        assert rig.run(P, label="rand30") == []
        s, cam, mesh, worker = rig.scene, rig.cam, rig.mesh, rig.worker
        worker.set_visibility_cull(True)
        mesh.project(None)
        reply = worker.post_message({"sort": {"modelViewProj": rig.mvp, "splatRenderCount": N, "splatSortCount": N}})
        mesh.use_sorter_result(worker, N)
        frame, _ = mesh.render()
        want_list = np.ascontiguousarray(reply["sortedIndexes"], dtype=np.uint32)
        assert 0 < want_list.size < N and frame.any()
    finally:
        rig.close()
        ctx.close()
    fx, fy = cam.focal()
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    eye = np.r_[np.asarray(cam.position, np.float64), 1.0]
    inv_cam = np.array([np.r_[(np.linalg.inv(np.asarray(t, np.float64).reshape(4, 4).T) @ eye)[:3], 1.0] for t in s.transforms]).reshape(-1)
    parts = [np.array([N, cases.W, cases.H, 2 * dyn.K, 0, 0, 0, 0], np.uint32), s.centers.astype(np.float32), s.cov.astype(np.float32), s.rgba,
             dyn.mesh_scene_indexes(s, P), s.sorter_scene, s.centres4.astype(np.int32), f32(cam.model_view()), f32(cam.projection), f32(cam.view),
             f32(cam.position), np.array([fx, fy], np.float32), f32(cam.sort_mvp()), f32(np.concatenate(s.transforms)), f32(inv_cam),
             np.array([1, 0] * dyn.K, np.uint32)]
    inp, exp, outp = (str(tmp_path / name) for name in ("in.bin", "expect.bin", "out.bin"))
    with open(inp, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())
    with open(exp, "wb") as f:
        f.write(np.ascontiguousarray(frame).tobytes() + want_list.tobytes())
    res = subprocess.run(["node", "dyn_vis_via_js.js", inp, exp, outp], cwd=NODE_DIR, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1]) == {"kept": int(want_list.size), "listEqual": True, "frameEqual": True}
    raw = np.fromfile(outp, dtype=np.uint8)
    nb = cases.W * cases.H * 4
    assert np.array_equal(raw[:nb].reshape(cases.H, cases.W, 4), frame) and np.array_equal(raw[nb:].view(np.uint32), want_list)
