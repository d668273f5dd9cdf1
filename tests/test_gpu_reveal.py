"""-m gpu: the scene reveal end to end in the Python mirror.  A 3000-splat scene arrives in three builds (the last one final); after
every build SplatMesh.update_visible_region measures the new splats on the device, every frame update_visible_region_fade_distance
advances the fade-in (SceneRevealMode.Default).  The state after every step equals reveal.py fed by the host model of
gs_mesh_bounds, bit for bit; frames at an early, a middle and the completed step are the frames a plain set_fade_in with those
values draws, and hold the fp32 raster oracle's tolerance with fade_in set."""
import math

import numpy as np
import pytest

import bounds_ref
import helpers
import oracle
from gaussiansplats3d_amd import Context, SplatMesh, camera, util
from gaussiansplats3d_amd.reveal import SceneRevealMode, VisibleRegion

pytestmark = pytest.mark.gpu
W, H, N = 160, 96, 3000
BUILDS = [(1000, False, 30), (2000, False, 30), (3000, True, 450)]       # (splats uploaded, finalBuild, frames that follow)


def _scene():
    scene = helpers.small_scene(N, 0, seed=77)
    center = scene.centers.mean(axis=0).astype(np.float32)
    near_first = np.argsort(np.linalg.norm(scene.centers - center, axis=1), kind="stable")    # the radius grows with every build
    scene.centers, scene.cov, scene.rgba = scene.centers[near_first], scene.cov[near_first], scene.rgba[near_first]
    return scene, center


def _draw(mesh, cam, order, count):
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, count)
    return mesh.render()[0]


def _oracle(scene, cam, order, count, fade=None):
    c, cov, rgba, sh = helpers.oracle_inputs(scene)
    ocam = oracle.make_camera(cam.model_view(), cam.projection, cam.position, cam.width, cam.height, sh_degree=0, sh_stored=0)
    if fade is not None:
        ocam.fade_in, ocam.fade_start = 1, fade[1]
        ocam.scene_center[:] = np.asarray(fade[0], np.float32).tolist()
    return oracle.render(ocam, c[:count], cov[:count], rgba[:count], sh, order)


def test_a_progressive_load_fades_in_as_the_reference_would():
    ctx = Context(0)
    scene, center = _scene()
    cam = camera.demo_camera("garden", W, H)
    ci = util.integer_centers(scene.centers)
    orders = {n: oracle.sort_indexes(np.arange(n, dtype=np.uint32), ci[:n], cam.sort_mvp()) for n, _, _ in BUILDS}
    mesh, plain = SplatMesh(ctx, N, 0), SplatMesh(ctx, N, 0)
    model = VisibleRegion()
    shots, done, start, complete_at = {}, 0, 0, None
    for b, (count, final, frames) in enumerate(BUILDS):
        for m in (mesh, plain):
            m.build(scene.centers[start:count], scene.cov[start:count], scene.rgba[start:count], start=start)
        region = mesh.update_visible_region(b > 0, [center] if b == 0 else None, final_build=final)
        model.update(b > 0, [center.tolist()], final,
                     lambda c, s=start, e=count: math.sqrt(bounds_ref.bounds(scene.centers, c, s, e - s)["max_dist_sq"]))
        assert region.calculated_scene_center == model.calculated_scene_center and region.state() == model.state(), (b, region.state(), model.state())
        assert mesh.last_build_splat_count == count
        for f in range(frames):
            region = mesh.update_visible_region_fade_distance(SceneRevealMode.Default)
            model.update_fade_distance(SceneRevealMode.Default)
            assert region.state() == model.state(), (b, f, region.state(), model.state())
            assert (mesh.fade_in is None) == bool(model.shader_fade_in_complete)
            if mesh.fade_in is not None:
                assert mesh.fade_in[1] == model.visible_region_fade_start_radius
            if b == 2 and complete_at is None and not region.visible_region_changing:
                complete_at = f
            shot = "early" if (b, f) == (0, frames - 1) else "middle" if (b, f) == (1, frames - 1) else \
                "complete" if (b == 2 and complete_at == f) else None
            if shot:
                fade = None if mesh.fade_in is None else (list(model.calculated_scene_center), model.visible_region_fade_start_radius)
                shots[shot] = (count, fade, _draw(mesh, cam, orders[count], count))
        start = count
    print("radii after the builds:", model.state(), "complete at frame", complete_at)
    assert complete_at is not None and set(shots) == {"early", "middle", "complete"}
    assert shots["early"][1] is not None and shots["middle"][1] is not None and shots["complete"][1] is None
    assert shots["middle"][1][1] > shots["early"][1][1] > 0.0

    never_faded = _draw(plain, cam, orders[N], N)                          # (plain holds all 3000 splats by now, and never faded)
    assert np.array_equal(shots["complete"][2], never_faded), "the completed fade-in must draw the un-faded frame"
    for name in ("early", "middle"):
        count, (c, radius), got = shots[name]
        plain.set_fade_in(c, radius)
        assert np.array_equal(got, _draw(plain, cam, orders[count], count)), f"{name}: not the frame set_fade_in({c}, {radius}) draws"
        fb, q, amb, _ = _oracle(scene, cam, orders[count], count, (c, radius))
        print(helpers.compare_frames(got, fb, amb, f"reveal {name}"))
        plain.set_fade_in(None)
        if name == "early":
            unfaded = _draw(plain, cam, orders[count], count)
            full = _oracle(scene, cam, orders[count], count)[1]
            assert np.abs(full.astype(int) - q.astype(int)).max() > 20, "fade-in should change the image"
            assert np.abs(unfaded.astype(int) - got.astype(int)).max() > 20, "fade-in should change the frame"
    fb, q, amb, _ = _oracle(scene, cam, orders[N], N)
    print(helpers.compare_frames(shots["complete"][2], fb, amb, "reveal complete"))
    mesh.dispose()
    plain.dispose()
    ctx.close()
