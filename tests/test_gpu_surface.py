"""-m gpu: the surface pass (gs_mesh_surface, csrc/tile_blend.hip k_surface) - per pixel the splat at which the front-to-back
transmittance of the last draw falls to a threshold, and that splat's window depth.

Hand-made scenes whose answer is known, a random scene held to the host model pixel by pixel (surface_ref.py: a validity check,
not an equality - the kernel's alpha goes through v_exp_f32), and EXACT invariances: the answer does not depend on the window, on
strips, on the list-bin size, on the storage order or on the draw mode (ids equal, depth bits equal)."""
import ctypes as C

import numpy as np
import pytest

import surface_cases as cases
import surface_ref as ref
from gaussiansplats3d_amd import Context, GsError, SplatMesh, camera
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
NONE = ref.NONE
W, H = 150, 90                        # 4.7 x 2.8 bins: the last bin and the last quadrant of both axes are partial


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def drawn(ctx, scene, cam, order=None, tile_rows=None, before_draw=None, **mesh_kw):
    mesh = SplatMesh(ctx, scene.count, scene.sh_degree, False, **mesh_kw)
    mesh.build(scene.centers, scene.cov, scene.rgba, scene.sh if scene.sh_degree else None)
    if before_draw:
        before_draw(mesh)
    mesh.set_camera(cam)
    order = cases.back_to_front(scene, cam) if order is None else order
    mesh.update_render_indexes(order, scene.count)
    mesh.render(tile_rows=tile_rows)
    return mesh


def same(a, b):
    """ids equal and depth bits equal"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# -- hand-made scenes at 64 x 64 ------------------------------------------------------------------------------------------------
def test_one_opaque_splat_is_the_surface_near_its_centre_and_nowhere_else(ctx):
    cam = cases.small_camera()
    scene = cases.one_opaque(cam)
    mesh = drawn(ctx, scene, cam)
    ids, depth = mesh.surface(0, 0, 64, 64)
    z = ref.window_depth(scene.centers, list(mesh._cam.view), list(mesh._cam.proj))
    assert (ids[30:34, 30:34] == 0).all() and np.abs(depth[30:34, 30:34].astype(np.float64) - z[0]).max() <= ref.DEPTH_TOL
    assert 0.9 < z[0] < 1.0
    for y, x in ((0, 0), (63, 63), (0, 63), (32, 2)):
        assert ids[y, x] == NONE and depth[y, x] == np.float32(1.0)
    assert ref.check_window(cases.draw_of(mesh, scene.centers), 0, 0, ids, depth, 0.5) == []
    mesh.dispose()


@pytest.mark.parametrize("tau, want", [(0.5, 1), (0.7, 0), (0.3, NONE)])
def test_two_layers_of_alpha_04(ctx, tau, want):
    """T = 0.6 after the near layer, 0.36 after the far one."""
    cam = cases.small_camera()
    scene = cases.two_layers(cam)
    mesh = drawn(ctx, scene, cam)
    ids, depth = mesh.surface(0, 0, 64, 64, tau)
    assert (ids == want).all()
    z = ref.window_depth(scene.centers, list(mesh._cam.view), list(mesh._cam.proj))
    assert np.abs(depth.astype(np.float64) - (1.0 if want == NONE else z[want])).max() <= (0.0 if want == NONE else ref.DEPTH_TOL)
    assert z[0] < z[1]
    assert ref.check_window(cases.draw_of(mesh, scene.centers), 0, 0, ids, depth, tau) == []
    mesh.dispose()


def test_an_empty_frame_has_no_surface(ctx):
    cam = cases.small_camera()
    scene = cases.behind_the_eye(cam)
    mesh = drawn(ctx, scene, cam)
    ids, depth = mesh.surface(0, 0, 64, 64)
    assert (ids == NONE).all() and (depth == np.float32(1.0)).all()
    mesh.dispose()


# -- a random scene against the model -------------------------------------------------------------------------------------------
class Frame:
    """helpers.small_scene(3000, 1, 5) drawn once at 150 x 90, its model input and its full-frame surface at 0.5: shared, unchanged."""

    def __init__(self, ctx):
        import oracle
        from gaussiansplats3d_amd import util
        self.cam = camera.demo_camera("garden", W, H)
        self.scene = cases.random_scene(5)
        self.order = oracle.sort_indexes(np.arange(self.scene.count, dtype=np.uint32), util.integer_centers(self.scene.centers), self.cam.sort_mvp())
        self.mesh = drawn(ctx, self.scene, self.cam, self.order)
        self.full = self.mesh.surface(0, 0, W, H, 0.5)
        self.draw = cases.draw_of(self.mesh, self.scene.centers)


@pytest.fixture(scope="module")
def frame(ctx):
    f = Frame(ctx)
    yield f
    f.mesh.dispose()


@pytest.mark.parametrize("tau", [0.5, 0.1])
def test_every_pixel_of_a_random_scene_is_valid_by_the_model(frame, tau):
    ids, depth = frame.full if tau == 0.5 else frame.mesh.surface(0, 0, W, H, tau)
    bad = ref.check_window(frame.draw, 0, 0, ids, depth, tau)
    assert bad == [], f"{len(bad)} invalid pixels, first: {bad[:3]}"
    hit = ids != NONE
    assert 0.2 < hit.mean() < 1.0 and (~hit).any(), "the scene must have surface and holes"
    assert np.unique(ids[hit]).shape[0] > 100
    # every id names a visible splat whose rect covers the pixel's tile
    d = frame.draw
    py, px = np.nonzero(hit)
    s = ids[hit]
    assert (s < frame.scene.count).all() and d.vis[s].all()
    r = d.rects[s]
    assert ((px // 16 >= (r[:, 0] & 0xFFFF)) & (px // 16 <= (r[:, 1] & 0xFFFF)) & (py // 16 >= (r[:, 0] >> 16)) & (py // 16 <= (r[:, 1] >> 16))).all()
    assert (depth[~hit] == np.float32(1.0)).all() and (depth[hit] < 1.0).all() and (depth[hit] > 0.0).all()


# -- exact invariances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0, y0, w, h", [(77, 41, 1, 1), (0, 0, 1, 1), (149, 89, 1, 1), (13, 7, 97, 61), (31, 31, 34, 34)])
def test_a_window_equals_the_same_pixels_of_the_full_frame(frame, x0, y0, w, h):
    got = frame.mesh.surface(x0, y0, w, h, 0.5)
    assert got[0].shape == (h, w) and same(got, (frame.full[0][y0:y0 + h, x0:x0 + w], frame.full[1][y0:y0 + h, x0:x0 + w]))


@pytest.mark.parametrize("rows", [(0, 2), (1, 4), (3, 6)])
def test_a_strip_draw_equals_the_full_frame_on_its_own_rows(ctx, frame, rows):
    mesh = drawn(ctx, frame.scene, frame.cam, frame.order, tile_rows=rows)
    y0, y1 = rows[0] * 16, min(rows[1] * 16, H)
    got = mesh.surface(0, y0, W, y1 - y0, 0.5)
    assert same(got, (frame.full[0][y0:y1], frame.full[1][y0:y1]))
    with pytest.raises(GsError, match="leaves the rows the last draw covered"):      # one row outside the strip
        mesh.surface(0, y0 - 1, W, 2, 0.5) if y0 else mesh.surface(0, y1 - 1, W, 2, 0.5)
    mesh.dispose()


@pytest.mark.parametrize("shift", [1, 3])
def test_the_list_bin_size_does_not_matter(ctx, frame, monkeypatch, shift):
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", str(shift))     # read when the mesh is created
    mesh = drawn(ctx, frame.scene, frame.cam, frame.order)
    assert mesh.last_stats().list_bin_px == 16 << shift
    assert same(mesh.surface(0, 0, W, H, 0.5), frame.full)
    mesh.dispose()


def test_upload_order_storage_equals_morton_storage(ctx, frame):
    mesh = drawn(ctx, frame.scene, frame.cam, frame.order, keep_order=True)
    assert same(mesh.surface(0, 0, W, H, 0.5), frame.full)
    mesh.dispose()


def test_the_draw_mode_does_not_matter(ctx, frame):
    mesh = drawn(ctx, frame.scene, frame.cam, frame.order, before_draw=lambda m: m.set_draw_mode(rop8=True))
    assert same(mesh.surface(0, 0, W, H, 0.5), frame.full)
    mesh.dispose()


# -- more than one batch of 256 entries -----------------------------------------------------------------------------------------
def pile_mesh(ctx, cam, count, opacity):
    scene = cases.pile(cam, count)
    mesh = drawn(ctx, scene, cam, order=np.arange(count, dtype=np.uint32), enable_optional_effects=True,
                 before_draw=lambda m: m.set_scenes(opacity=[opacity]))
    return scene, mesh


def test_a_pile_of_faint_splats_crosses_in_the_second_batch(ctx):
    """3000 coincident splats of alpha 0.51 / 255 = 0.002: 0.998 ^ k falls to 0.5 at k = 347."""
    cam = cases.small_camera()
    scene, mesh = pile_mesh(ctx, cam, 3000, 0.51)
    ids, depth = mesh.surface(0, 0, 64, 64, 0.5)
    d = cases.draw_of(mesh, scene.centers)
    assert ref.check_window(d, 0, 0, ids, depth, 0.5) == []
    assert (ids != NONE).all()
    k = np.array([cases.entry_index(d, x, y, int(ids[y, x])) for y, x in ((32, 32), (0, 0), (63, 63), (17, 48))])
    print("crossing entries:", k)
    assert (k >= 256).all() and (k >= 340).all() and (k <= 355).all()
    mesh.dispose()


def test_a_pile_too_faint_to_cross_has_no_surface(ctx):
    """800 coincident splats of alpha 0.1275 / 255 = 0.0005: T ends at 0.67."""
    cam = cases.small_camera()
    scene, mesh = pile_mesh(ctx, cam, 800, 0.1275)
    ids, depth = mesh.surface(0, 0, 64, 64, 0.5)
    assert (ids == NONE).all() and (depth == np.float32(1.0)).all()
    assert ref.check_window(cases.draw_of(mesh, scene.centers), 0, 0, ids, depth, 0.5) == []
    mesh.dispose()


# -- destination depth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dest", ["none", "fp32", "unorm24"])
def test_splats_behind_an_occluder_are_not_surface(ctx, dest):
    cam = cases.small_camera()
    scene = cases.occluded(cam)
    z = ref.window_depth(scene.centers, np.asarray(cam.model_view()), np.asarray(cam.projection))
    mid = np.float32(0.5 * (z[0] + z[1]))
    assert z[0] + 5e-3 < mid < z[1] - 5e-3                  # well clear of both layers (a 24-bit step is 6e-8)
    plane = np.full((64, 64), mid, dtype=np.float32)
    setup = None if dest == "none" else (lambda m: m.set_destination(depth=plane, depth_unorm24=dest == "unorm24"))
    mesh = drawn(ctx, scene, cam, before_draw=setup)
    ids, depth = mesh.surface(0, 0, 64, 64, 0.5)
    if dest == "none":
        assert (ids == 1).all() and np.abs(depth.astype(np.float64) - z[1]).max() <= ref.DEPTH_TOL
    else:
        assert (ids == NONE).all() and (depth == np.float32(1.0)).all()      # T stays at 0.6: the opaque layer is hidden
        ids7, _ = mesh.surface(0, 0, 64, 64, 0.7)
        assert (ids7 == 0).all()                                               # ... and the near layer still counts
    model = cases.draw_of(mesh, scene.centers, dest_depth=None if dest == "none" else plane, unorm24=dest == "unorm24")
    assert ref.check_window(model, 0, 0, ids, depth, 0.5) == []
    mesh.dispose()


# -- per-scene transforms -------------------------------------------------------------------------------------------------------
def test_dynamic_scenes_report_the_depth_of_their_own_transform(ctx):
    cam = cases.small_camera()
    scene, scene_idx, transforms = cases.two_scenes(cam)
    mesh = SplatMesh(ctx, scene.count, 0, False, dynamic_mode=True)
    mesh.build(scene.centers, scene.cov, scene.rgba, None, scene_indexes=scene_idx)
    mesh.set_scenes(transforms=transforms, camera_position=cam.position)
    mesh.set_camera(cam)
    mesh.update_render_indexes(np.array([0, 1], dtype=np.uint32), 2)          # scene 0's splat is the far one
    mesh.render()
    ids, depth = mesh.surface(0, 0, 64, 64)
    c = mesh._cam
    z = ref.window_depth(scene.centers, list(c.view), list(c.proj), view_matrix16=list(c.view_matrix), transforms=transforms,
                         scene_of_splat=scene_idx)
    static = ref.window_depth(scene.centers, list(c.view), list(c.proj))
    assert abs(z[0] - z[1]) > 1e-3 and abs(z[0] - static[0]) > 1e-3 and abs(z[1] - static[1]) > 1e-3
    for s in (0, 1):
        assert (ids == s).sum() > 20, f"scene {s}'s splat is nowhere the surface"
        assert np.abs(depth[ids == s].astype(np.float64) - z[s]).max() <= ref.DEPTH_TOL
    assert (ids == NONE).any()
    mesh.dispose()


# -- outputs --------------------------------------------------------------------------------------------------------------------
def test_device_outputs_equal_host_outputs(frame):
    import torch
    x0, y0, w, h = 5, 3, 140, 80
    ids_t = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    z_t = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    none_ids, none_z = frame.mesh.surface(x0, y0, w, h, 0.5, ids_device_ptr=ids_t.data_ptr(), depth_device_ptr=z_t.data_ptr())
    assert none_ids is None and none_z is None
    frame.mesh.ctx.synchronize()
    want = (frame.full[0][y0:y0 + h, x0:x0 + w], frame.full[1][y0:y0 + h, x0:x0 + w])
    assert same((ids_t.cpu().numpy().view(np.uint32), z_t.cpu().numpy()), want)
    # one plane on the host, the other on the device
    z_t.fill_(-1.0)
    torch.cuda.synchronize()
    ids, none_z = frame.mesh.surface(x0, y0, w, h, 0.5, depth_device_ptr=z_t.data_ptr())
    frame.mesh.ctx.synchronize()
    assert none_z is None and same((ids, z_t.cpu().numpy()), want)


def test_untouched_lists_of_poisoned_allocations_read_none(monkeypatch):
    cam = cases.small_camera()
    scene = cases.one_opaque(cam, offset_px=(-16.0, -16.0))  # inside the first of the four 32-px lists: the other three stay untouched
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    clean_ctx = Context(0)
    mesh = drawn(clean_ctx, scene, cam)
    want = mesh.surface(0, 0, 64, 64)
    mesh.dispose()
    clean_ctx.close()
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", "0xFF")      # (read at every allocation: stays set for the whole test)
    pctx = Context(0)
    mesh = drawn(pctx, scene, cam)
    counts = mesh.bin_entry_counts()
    assert (counts == 0).any() and (counts > 0).any()
    got = mesh.surface(0, 0, 64, 64)
    assert same(got, want)
    empty = np.repeat(np.repeat(counts == 0, 32, axis=0), 32, axis=1)[:64, :64]
    assert (got[0][empty] == NONE).all() and (got[1][empty] == np.float32(1.0)).all()
    mesh.dispose()
    pctx.close()


# -- refusals -------------------------------------------------------------------------------------------------------------------
def refused(mesh, x0, y0, w, h, tau, needle, ids=True, depth=True, ids_dev=None, depth_dev=None):
    """The call fails with GS_ERR_INVALID, gs_last_error names the cause, and the host outputs keep what they held."""
    a = np.full((max(h, 1), max(w, 1)), 0xABCD1234, dtype=np.uint32)
    b = np.full((max(h, 1), max(w, 1)), -7.5, dtype=np.float32)
    st = mesh.lib.gs_mesh_surface(mesh.handle, x0, y0, w, h, C.c_float(tau), a.ctypes.data if ids else None, b.ctypes.data if depth else None,
                                  C.c_void_p(ids_dev) if ids_dev else None, C.c_void_p(depth_dev) if depth_dev else None)
    msg = mesh.lib.gs_last_error().decode()
    assert st == L.GS_ERR_INVALID, (st, msg)
    assert needle in msg, msg
    assert (a == 0xABCD1234).all() and (b == np.float32(-7.5)).all()


def test_refusals(ctx):
    import torch
    cam = cases.small_camera()
    scene = cases.two_layers(cam)
    mesh = SplatMesh(ctx, scene.count, 0, False).build(scene.centers, scene.cov, scene.rgba, None)
    refused(mesh, 0, 0, 8, 8, 0.5, "no draw yet")
    mesh.dispose()
    mesh = drawn(ctx, scene, cam, tile_rows=(1, 3))                            # rows 16 .. 47
    for tau in (0.0, 1.0, -0.25, 1.5, float("nan")):
        refused(mesh, 0, 16, 8, 8, tau, "threshold")
    refused(mesh, 0, 16, 0, 8, 0.5, "window is empty")
    refused(mesh, 0, 16, 8, 0, 0.5, "window is empty")
    refused(mesh, 60, 16, 5, 8, 0.5, "leaves the rows the last draw covered")
    refused(mesh, 0, 15, 8, 8, 0.5, "leaves the rows the last draw covered")
    refused(mesh, 0, 41, 8, 8, 0.5, "leaves the rows the last draw covered")
    refused(mesh, 0xFFFFFFF0, 16, 0x20, 8, 0.5, "leaves the rows the last draw covered")
    refused(mesh, 0, 16, 8, 8, 0.5, "all four outputs are NULL", ids=False, depth=False)
    dev = torch.zeros(64, dtype=torch.int32, device="cuda")
    refused(mesh, 0, 16, 8, 8, 0.5, "id plane on the host OR on the device", ids_dev=dev.data_ptr())
    refused(mesh, 0, 16, 8, 8, 0.5, "depth plane on the host OR on the device", depth_dev=dev.data_ptr())
    ids, _ = mesh.surface(0, 16, 64, 32, 0.5)                                  # (the mesh itself is fine)
    assert (ids == 1).all()
    mesh.project(tile_rows=(1, 3))
    refused(mesh, 0, 16, 8, 8, 0.5, "gs_mesh_project is pending")
    mesh.render(tile_rows=(1, 3))
    mesh.set_destination(depth=np.full((64, 64), 0.5, dtype=np.float32))
    refused(mesh, 0, 16, 8, 8, 0.5, "destination changed since the last draw")
    mesh.set_destination()
    ids, _ = mesh.surface(0, 16, 64, 32, 0.5)
    assert (ids == 1).all()
    mesh.dispose()


# -- the depth is the vertex stage's own -----------------------------------------------------------------------------------------
def test_the_depth_has_the_bits_the_vertex_stage_wrote(ctx, frame):
    """Under an fp32 destination depth k_project leaves 0.5 * ndc.z + 0.5 of every visible splat in a plane of its own (debug read
    13): the pass recomputes it after the walk and must arrive at the same bits.  The destination is 1.0 everywhere, so nothing is
    hidden and the answer is the frame's own as well."""
    plane = np.ones((H, W), dtype=np.float32)
    mesh = drawn(ctx, frame.scene, frame.cam, frame.order, before_draw=lambda m: m.set_destination(depth=plane))
    ids, depth = mesh.surface(0, 0, W, H, 0.5)
    assert same((ids, depth), frame.full)
    z = mesh.debug_depths()
    hit = ids != NONE
    assert hit.sum() > 1000 and np.array_equal(depth[hit].view(np.uint32), z[ids[hit]].view(np.uint32))
    mesh.dispose()


def test_the_depth_of_dynamic_scenes_has_the_bits_the_vertex_stage_wrote(ctx):
    cam = cases.small_camera()
    scene, scene_idx, transforms = cases.two_scenes(cam)
    mesh = SplatMesh(ctx, scene.count, 0, False, dynamic_mode=True)
    mesh.build(scene.centers, scene.cov, scene.rgba, None, scene_indexes=scene_idx)
    mesh.set_scenes(transforms=transforms, camera_position=cam.position)
    mesh.set_destination(depth=np.ones((64, 64), dtype=np.float32))
    mesh.set_camera(cam)
    mesh.update_render_indexes(np.array([0, 1], dtype=np.uint32), 2)
    mesh.render()
    ids, depth = mesh.surface(0, 0, 64, 64)
    z = mesh.debug_depths()
    for s in (0, 1):
        assert (ids == s).sum() > 20 and (depth[ids == s].view(np.uint32) == z[s:s + 1].view(np.uint32)[0]).all()
    mesh.dispose()


# -- the Node seam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", ["identity", "moved"])
def test_the_node_raycaster_returns_the_hit_python_sees(ctx, tmp_path, placed):
    """node/Raycaster.mjs on the two-layer scene: one hit, Python's splat, and its origin is camera.unproject's WORLD point - also
    when the mesh carries a model matrix (translated and scaled): the origin is then not the mesh-local point, it lies on the
    camera's world-space ray, and the model matrix takes the local point to it."""
    import json
    import os
    import shutil
    import subprocess
    assert shutil.which("node") is not None, "node is part of the toolchain: the Node seam cannot go untested"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cam = cases.small_camera()
    scene = cases.two_layers(cam)
    model = None if placed == "identity" else cases.matrix16(0.0, (0.3, -0.2, 0.5), 1.5)
    order = cases.back_to_front(scene, cam)
    mesh = SplatMesh(ctx, scene.count, 0, False).build(scene.centers, scene.cov, scene.rgba, None)
    mesh.set_camera(cam, mesh_world=model)
    mesh.update_render_indexes(order, scene.count)
    mesh.render()
    sx, sy = 40.3, 20.7                                      # pointer position, y down: pixel (40, 43) of the GL frame
    px, py = 40, 43
    ids, depth = mesh.surface(px, py, 1, 1)
    c = mesh._cam
    world = camera.unproject(px + 0.5, py + 0.5, depth[0, 0], 64, 64, list(c.proj), list(c.view_matrix))
    local = camera.unproject(px + 0.5, py + 0.5, depth[0, 0], 64, 64, list(c.proj), list(c.view))
    assert ids[0, 0] == 1
    if model is not None:
        m = np.asarray(model).reshape(4, 4).T
        assert np.abs(world - local).max() > 0.3            # the two spaces are far apart ...
        assert np.abs(m[:3, :3] @ local + m[:3, 3] - world).max() <= 1e-5 * np.abs(world).max()   # ... and the model matrix joins them
    job = {"centers": scene.centers.ravel().tolist(), "cov": scene.cov.ravel().tolist(), "rgba": scene.rgba.ravel().tolist(),
           "order": order.tolist(), "modelView": list(c.view), "viewMatrix": list(c.view_matrix), "proj": list(c.proj),
           "camPos": list(c.cam_pos), "focal": list(c.focal), "width": 64, "height": 64,
           "matrixWorld": np.asarray(cam.matrix_world).tolist(), "screen": [sx, sy]}
    (tmp_path / "in.json").write_text(json.dumps(job))
    subprocess.check_call(["make", "-C", os.path.join(root, "node")], stdout=subprocess.DEVNULL)
    out = subprocess.check_output(["node", "--no-warnings", "--experimental-loader", os.path.join(root, "oracle", "three_loader.mjs"),
                                   os.path.join(root, "node", "surface_via_js.mjs"), str(tmp_path / "in.json")], text=True, timeout=120)
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got["hits"]) == 1 and got["noneAt03"] == 0
    hit = got["hits"][0]
    assert hit["splatIndex"] == int(ids[0, 0]) and hit["pixel"] == {"x": px, "y": py}
    assert np.float32(hit["depth"]) == depth[0, 0]
    assert np.abs(np.asarray(hit["origin"]) - world).max() <= 1e-5 * np.abs(world).max()
    assert np.allclose(got["rayOrigin"], cam.position, atol=1e-9)
    assert np.allclose(hit["normal"], -np.asarray(got["direction"]), atol=1e-12)
    assert abs(hit["distance"] - np.linalg.norm(world - cam.position)) <= 1e-5 * hit["distance"]
    # the hit lies on the world-space ray through the pointer position (the pixel's centre is within a pixel of it: 0.3 px of
    # 68.6 px focal length at this distance)
    along = np.asarray(got["rayOrigin"]) + np.asarray(got["direction"]) * hit["distance"]
    assert np.abs(along - world).max() < 0.01 * hit["distance"]
    mesh.dispose()
