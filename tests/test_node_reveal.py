"""-m gpu: the scene reveal through the JavaScript drop-in (node/SplatMesh.mjs, driven by node/reveal_via_js.mjs): a progressive load -
build, update builds, a final build, updateVisibleRegionFadeDistance(mode) per frame.  The state after every build and frame equals
reveal.py fed by the host model of gs_mesh_bounds, the frames equal the Python mirror's bit for bit, SceneRevealMode.Instant and a
mesh whose per-frame method is never called draw the un-faded frame, and computeBoundingBox answers as the Python mirror does."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounds_ref
import helpers
import oracle
from gaussiansplats3d_amd import Context, SplatMesh, camera, util
from gaussiansplats3d_amd.reveal import SceneRevealMode, VisibleRegion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 160, 96, 3000
BUILDS = [(1000, False, 12), (2000, False, 12), (3000, True, 40)]        # (splats loaded, finalBuild, frames that follow)
BOX_SCENE = {"position": [1.0, 2.0, 3.0], "scale": [2.0, 1.0, 0.5]}


def _frame(path):
    return np.fromfile(path, np.uint8).reshape(H, W, 4)


def test_the_drop_in_reveals_a_progressive_load_as_the_python_mirror_does(tmp_path):
    assert shutil.which("node") is not None, "node is part of the toolchain: the Node seam cannot go untested"
    scene = helpers.small_scene(N, 0, seed=78)
    center = scene.centers.mean(axis=0).astype(np.float32)
    near_first = np.argsort(np.linalg.norm(scene.centers - center, axis=1), kind="stable")
    c, cov, rgba = scene.centers[near_first], scene.cov[near_first], scene.rgba[near_first]
    cam = camera.demo_camera("garden", W, H)
    ci = util.integer_centers(c)
    orders = {n: oracle.sort_indexes(np.arange(n, dtype=np.uint32), ci[:n], cam.sort_mvp()) for n, _, _ in BUILDS}
    job = {"centers": c.reshape(-1).astype(np.float64).tolist(), "cov": cov.reshape(-1).astype(np.float64).tolist(),
           "rgba": rgba.reshape(-1).tolist(), "sceneCenter": center.astype(np.float64).tolist(), "mode": SceneRevealMode.Default,
           "builds": [{"count": n, "finalBuild": final, "frames": frames, "order": orders[n].tolist()} for n, final, frames in BUILDS],
           "width": W, "height": H, "focal": list(cam.focal(1.0)), "matrixWorld": np.asarray(cam.matrix_world, np.float64).reshape(-1).tolist(),
           "view": np.asarray(cam.view, np.float64).reshape(-1).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(-1).tolist(),
           "boxScene": BOX_SCENE}
    (tmp_path / "in.json").write_text(json.dumps(job))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "node")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(ROOT, "node", "reveal_via_js.mjs"), str(tmp_path / "in.json"), str(tmp_path)],
                                  cwd=os.path.join(ROOT, "tests"), text=True, timeout=300)
    got = json.loads(out.strip().splitlines()[-1])

    # the same load through the Python mirror, and through reveal.py fed by the host model
    ctx = Context(0)
    mesh, model = SplatMesh(ctx, N, 0), VisibleRegion()
    rows, start = iter(got["rows"]), 0
    for b, (count, final, frames) in enumerate(BUILDS):
        mesh.build(c[start:count], cov[start:count], rgba[start:count], start=start)
        region = mesh.update_visible_region(b > 0, [center] if b == 0 else None, final_build=final)
        model.update(b > 0, [center.tolist()], final, lambda p, s=start, e=count: math.sqrt(bounds_ref.bounds(c, p, s, e - s)["max_dist_sq"]))
        assert next(rows) == model.calculated_scene_center + model.state() == region.calculated_scene_center + region.state(), b
        for f in range(frames):
            region = mesh.update_visible_region_fade_distance(SceneRevealMode.Default)
            model.update_fade_distance(SceneRevealMode.Default)
            assert next(rows) == model.state() == region.state(), (b, f)
        assert mesh.fade_in is not None, "the fade-in is still running at every shot of this script"
        mesh.set_camera(cam)
        mesh.update_render_indexes(orders[count], count)
        assert np.array_equal(_frame(tmp_path / f"shot{b}.u8"), mesh.render()[0]), f"frame after build {b} differs from the Python mirror's"
        start = count
    mesh.set_fade_in(None)
    mesh.set_camera(cam)
    unfaded = mesh.render()[0]
    assert np.array_equal(_frame(tmp_path / "instant.u8"), unfaded), "SceneRevealMode.Instant must draw the un-faded frame"
    assert np.array_equal(_frame(tmp_path / "uncalled.u8"), unfaded), "a mesh whose fade distance is never updated must draw un-faded"
    assert np.abs(_frame(tmp_path / "shot2.u8").astype(int) - unfaded.astype(int)).max() > 20, "the fade-in should change the frame"

    lo, hi = mesh.compute_bounding_box(False)
    for key in ("boxPlain", "boxTransformed", "boxScene0"):                     # identity transform: every variant is this box
        assert got[key] == {"min": lo.tolist(), "max": hi.tolist()}, key
    assert got["badIndex"] == "SplatMesh::computeBoundingBox() -> Invalid scene index."
    # a static transform: the plain box is the centres', the transformed one what a mirror holding the baked centres answers
    baked = bounds_ref.transformed(c, [got["movedTransform"]]).astype(np.float32)
    moved = SplatMesh(ctx, N, 0).build(baked, cov, rgba)
    lo2, hi2 = moved.compute_bounding_box(True)
    assert got["movedTransformed"] == {"min": lo2.tolist(), "max": hi2.tolist()}
    assert got["movedPlain"] == {"min": lo.tolist(), "max": hi.tolist()}
    assert got["movedRadius"] == moved.update_visible_region(False, [center]).max_splat_distance_from_scene_center
    for m in (mesh, moved):
        m.dispose()
    ctx.close()
