"""-m gpu: SplatRenderMode.TwoD on the device (csrc/project_2d.hip, csrc/tile_blend_2d.hip) against the host model
(tests/surfel_ref.py) on the cases of tests/surfel_cases.py.

Tolerances.  Records: pixel positions within 3e-3 px, rows of vT and of the quad's inverse basis within 5e-4 of the row's norm, the
colour words equal (the figures the 3D vertex-stage check holds the engine to against a real GL; the model and the kernel share
operation order and neither contracts, so they sit far inside them).  Frames: every channel of every non-ambiguous pixel within one
8-bit step of the model's fp32 composite rounded once - the project's standing figure for its shaders' fp32 restatement; the kernel
differs from the model only in exp's last bit and in the T <= 1e-4 retirement.
"""
import numpy as np
import pytest

import helpers
import surfel_cases
import surfel_ref
from gaussiansplats3d_amd import Context, GsError, SplatMesh, camera, create_sort_worker, util
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _mesh(ctx, case, capacity=None, **kw):
    n = case["centers"].shape[0]
    sh8 = case["sh8_range"] is not None
    mesh = SplatMesh(ctx, capacity or n, case["sh_degree"], render_mode_2d=True, dynamic_mode=case["transforms"] is not None,
                     enable_optional_effects=case["opacity"] is not None, spherical_harmonics_8bit=sh8, **kw)
    mesh.build(case["centers"], None, case["rgba"], case["sh"], scales=case["scales"], rotations=case["rotations"],
               scene_indexes=case["scene_idx"])
    if case["transforms"] is not None or case["opacity"] is not None or sh8:
        mesh.set_scenes(transforms=case["transforms"], camera_position=case["camera"].position, opacity=case["opacity"],
                        visible=case["visible"], sh8_range=[case["sh8_range"]] if sh8 else None)
    if case["fade"] is not None:
        mesh.set_fade_in(*case["fade"])
    mesh.set_camera(case["camera"], focal_adjustment=1.0 / float(case["inv_focal_adj"]))
    return mesh


def _draw(ctx, case, order, dest=None, **kw):
    mesh = _mesh(ctx, case, **kw)
    if dest:
        mesh.set_destination(depth=dest["dest_depth"], rgba=dest["dest_rgba"], depth_unorm24=dest["depth_unorm24"])
    mesh.update_render_indexes(order, len(order))
    frame, stats = mesh.render()
    return mesh, frame, stats


def _hold_frame(got, out, label):
    clean = out["covered"] & ~out["ambiguous"]
    diff = np.abs(got.astype(int) - out["frame"].astype(int))
    print(f"{label}: covered {int(out['covered'].sum())}, compared {int(clean.sum())}, worst step {int(diff[clean].max(initial=0))}, "
          f"equal share {float((diff[clean] == 0).mean()) if clean.any() else 1.0:.4f}")
    assert (diff[clean] <= 1).all(), label
    untouched = ~out["covered"]
    assert np.array_equal(got[untouched], out["frame"][untouched]), label + ": pixels no quad reaches"


@pytest.mark.parametrize("name", surfel_cases.VERTEX_CASES)
def test_records_against_the_model(ctx, name):
    case = surfel_cases.vertex_case(name)
    v = surfel_ref.vertex(case)
    mesh, _, stats = _draw(ctx, case, np.arange(2000, dtype=np.uint32))
    recs, rects, vis = mesh.debug_records_2d()
    assert np.array_equal(vis, v["visible"]), f"visibility differs at {np.flatnonzero(vis != v['visible'])[:8]}"
    assert stats.visible_splats == int(vis.sum())
    want = surfel_ref.records(v)
    g, w = recs[vis, :17].view(np.float32), want[vis, :17].view(np.float32)
    for label, sl, rel in (("Tu", slice(0, 3), True), ("Tv", slice(3, 6), True), ("Tw", slice(6, 9), True), ("inverse basis", slice(13, 17), True),
                           ("quad centre px", slice(11, 13), False)):
        d = np.abs(g[:, sl] - w[:, sl])
        d = d / np.linalg.norm(w[:, sl], axis=1, keepdims=True) if rel else d
        print(f"{name} {label}: worst {'relative' if rel else 'px'} distance {float(d.max()):.3e}")
        assert (d <= (5e-4 if rel else 3e-3)).all(), label
    qc = np.abs(g[:, 9:11] - w[:, 9:11])                         # vQuadCenter: pixels in the AABB branch, NDC in the other
    assert (qc <= np.where(v["branch"][vis, None] == 1, 3e-3, 3e-3 / 144.0)).all()
    # colour and opacity: the 3D check's unorm16 figure, one unit per channel (identical without SH)
    chan = lambda r: np.stack([r[:, 17] & 0xFFFF, r[:, 17] >> 16, r[:, 18] & 0xFFFF, r[:, 18] >> 16], 1).astype(np.int64)   # noqa: E731
    cd = np.abs(chan(recs[vis]) - chan(want[vis]))
    print(f"{name} colour words: worst distance {int(cd.max())} / 65535, equal share {float((cd == 0).mean()):.5f}")
    assert (cd <= 1).all() and (case["sh_degree"] > 0 or (cd == 0).all())
    assert np.array_equal(rects[vis], (v["rect"][vis, 0] | (v["rect"][vis, 1] << 16))[:, None] * np.array([1, 0], np.uint32)
                          + (v["rect"][vis, 2] | (v["rect"][vis, 3] << 16))[:, None] * np.array([0, 1], np.uint32))
    assert mesh.view_share()["instance"] & 8
    mesh.dispose()


@pytest.mark.parametrize("sh_degree,sh8", [(2, False), (1, False), (2, True)])
def test_sh_colour_is_the_base_stage_s(ctx, sh_degree, sh8):
    """SH 1 / 2 and 8-bit SH come with the base stage: a surfel mesh and a 3D mesh over the same centres, colours and SH leave the
    same colour words for every splat both of them draw."""
    scene = helpers.small_scene(2000, sh_degree, seed=77)
    cam = camera.demo_camera("garden", 256, 144)
    rng = np.random.default_rng(3)
    sc = np.exp(rng.normal(np.log(0.03), 0.6, size=(2000, 3))).astype(np.float32)
    sh = scene.sh
    kw = {}
    if sh8:
        sh = np.clip(np.floor((np.clip(scene.sh.astype(np.float32), -0.9, 1.1) + 0.9) / 2.0 * 255.0), 0, 255).astype(np.uint8)
        kw = dict(spherical_harmonics_8bit=True)
    flat = SplatMesh(ctx, 2000, sh_degree, render_mode_2d=True, **kw)
    flat.build(scene.centers, None, scene.rgba, sh, scales=sc, rotations=surfel_cases._quats(rng, 2000))
    full = SplatMesh(ctx, 2000, sh_degree, **kw)
    full.build(scene.centers, scene.cov, scene.rgba, sh)
    for mesh in (flat, full):
        if sh8:
            mesh.set_scenes(sh8_range=[(-0.9, 1.1)])
        mesh.set_camera(cam)
        mesh.update_render_indexes(np.arange(2000, dtype=np.uint32), 2000)
        mesh.render()
    r2, _, v2 = flat.debug_records_2d()
    r3, _, v3 = full.debug_records()
    both = v2 & v3
    assert both.sum() > 500
    assert np.array_equal(r2[both, 17], r3[both, 6]) and np.array_equal(r2[both, 18] & 0xFFFF, r3[both, 7] & 0xFFFF)
    flat.dispose()
    full.dispose()


@pytest.mark.parametrize("name", surfel_cases.FRAME_CASES)
def test_frame_cases_against_the_model(ctx, name):
    case, order, dest = surfel_cases.frame_case(name)
    out = surfel_ref.render(case, order, **dest)
    mesh, got, stats = _draw(ctx, case, order, dest)
    _hold_frame(got, out, name)
    assert stats.splats_walked > 0 and stats.halves_evaluated == 2 * stats.splats_walked and stats.entries_scanned > 0
    mesh.dispose()


@pytest.mark.parametrize("name", surfel_cases.DESIGNED_CASES)
def test_designed_cases_against_the_model(ctx, name):
    case, order, dest = surfel_cases.designed_case(name)
    out = surfel_ref.render(case, order, **dest)
    mesh, got, stats = _draw(ctx, case, order, dest)
    _hold_frame(got, out, name)
    if name.startswith("list_"):                                  # translucent, nothing saturates: every entry is walked
        assert stats.tile_entries == int(name[5:]) and stats.entries_scanned >= stats.tile_entries
    mesh.dispose()


def test_poisoned_allocations(ctx, monkeypatch):
    case, order, dest = surfel_cases.frame_case("translucent")
    out = surfel_ref.render(case, order)
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", "0xFF")
    mesh, got, _ = _draw(ctx, case, order)
    _hold_frame(got, out, "poisoned")
    mesh.dispose()


def test_host_list_bound_sorter_and_culled_sort_draw_the_same_bits(ctx):
    case, _, _ = surfel_cases.frame_case("mixed_branches")
    n = case["centers"].shape[0]
    cam = case["camera"]
    ci = util.integer_centers(case["centers"])
    worker = create_sort_worker(ctx, n)
    worker.post_message({"centers": ci, "range": {"from": 0, "to": n - 1, "count": n}})
    reply = worker.post_message({"sort": {"modelViewProj": cam.sort_mvp(), "splatRenderCount": n, "splatSortCount": n}})
    order = reply["sortedIndexes"]
    mesh = _mesh(ctx, case)
    mesh.update_render_indexes(order, n)
    a, _ = mesh.render()
    worker.sort_on_device(cam.sort_mvp(), n)
    mesh.use_sorter_result(worker, n)
    worker.sort_on_device(cam.sort_mvp(), n)                     # (bound from this sort on)
    b, _ = mesh.render()
    worker.set_visibility_cull(True)
    mesh.project()
    worker.sort_on_device(cam.sort_mvp(), n)
    c, stats = mesh.render()
    assert a.any() and np.array_equal(a, b) and np.array_equal(a, c)
    out = surfel_ref.render(case, order)
    _hold_frame(a, out, "sorter order")
    worker.terminate()
    mesh.dispose()


def test_distances_bounds_and_trees_work_unchanged(ctx):
    case = surfel_cases.vertex_case("sh0")
    n = 2000
    flat = _mesh(ctx, case)
    full = SplatMesh(ctx, n, 0)
    full.build(case["centers"], np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (n, 1)), case["rgba"])
    mvp = case["camera"].sort_mvp()
    d2, d3 = np.empty(n, np.int32), np.empty(n, np.int32)
    flat.compute_distances_on_gpu(mvp, out=d2)
    full.compute_distances_on_gpu(mvp, out=d3)
    assert np.array_equal(d2, d3) and d2.any()
    b2, b3 = flat.bounds(0, n, (0, 0, 0)), full.bounds(0, n, (0, 0, 0))
    assert b2["count"] == n and np.array_equal(b2["min"], b3["min"]) and b2["max_dist_sq"] == b3["max_dist_sq"]
    bound, boxes, _ = flat.debug_cull_planes()                   # the bound: the largest squared scale of the stored tuple
    t = case["tuples"]
    assert np.array_equal(bound, np.maximum(np.maximum(t[:, 0] * t[:, 0], t[:, 1] * t[:, 1]), t[:, 2] * t[:, 2]))
    from gaussiansplats3d_amd.splat_tree import SplatTree
    tree = SplatTree(ctx)
    tree.process_splat_mesh(case["centers"])
    assert tree.info().splats == n
    tree.dispose()
    flat.dispose()
    full.dispose()


def test_remove_reorder_resize_equal_a_fresh_mesh(ctx):
    case, order, _ = surfel_cases.frame_case("opaque")
    n = case["centers"].shape[0]
    cam = case["camera"]
    half = n // 2

    def frame_of(mesh, idx):
        mesh.set_camera(cam)
        mesh.update_render_indexes(idx, len(idx))
        return mesh.render()[0]
    fresh = SplatMesh(ctx, n, 0, render_mode_2d=True)
    fresh.build(case["centers"], None, case["rgba"], scales=case["scales"], rotations=case["rotations"])
    want_all = frame_of(fresh, order)
    # two uploads folded into one run, then a larger capacity: the full frame
    m = SplatMesh(ctx, n, 0, render_mode_2d=True)
    for a, b in ((0, half), (half, n)):
        m.build(case["centers"][a:b], None, case["rgba"][a:b], scales=case["scales"][a:b], rotations=case["rotations"][a:b], start=a)
    m.reorder()
    assert np.array_equal(frame_of(m, order), want_all)
    m.resize(n + 300)
    assert np.array_equal(frame_of(m, order), want_all)
    r_resized = m.debug_records_2d()[0]
    assert np.array_equal(r_resized, fresh.debug_records_2d()[0])
    # the first upload removed: the frame of a fresh mesh holding the second one
    m2 = SplatMesh(ctx, n, 0, render_mode_2d=True)
    for a, b in ((0, half), (half, n)):
        m2.build(case["centers"][a:b], None, case["rgba"][a:b], scales=case["scales"][a:b], rotations=case["rotations"][a:b], start=a)
    m2.remove([(0, half)])
    rest = SplatMesh(ctx, n, 0, render_mode_2d=True)
    rest.build(case["centers"][half:], None, case["rgba"][half:], scales=case["scales"][half:], rotations=case["rotations"][half:])
    sub = (order[order >= half] - half).astype(np.uint32)
    got, want = frame_of(m2, sub), frame_of(rest, sub)
    assert want.any() and np.array_equal(got, want)
    for mesh in (fresh, m, m2, rest):
        mesh.dispose()


@pytest.mark.parametrize("fmt", ["ksplat", "ply"])
def test_device_decode_equals_host_fill_plus_upload(ctx, fmt):
    """gs_mesh_upload_asset into a surfel mesh stores (sx, sy, 1, qx, qy, qz): the planes a host fill of scales / rotations plus
    an upload leaves, seen through everything that reads them - the bound plane, the block boxes, the records and the frame."""
    from gaussiansplats3d_amd import assets
    n = 1500
    c, s_, r, rgba = surfel_cases.surfel_scene(n, 4400, 0.04, 0.8)
    wxyz = np.concatenate([r[:, 3:], r[:, :3]], axis=1) * np.float32(1.7)          # not normalised in the file
    wxyz[::3] *= -1.0                                                             # ... and w < 0 for a third of them
    if fmt == "ksplat":
        data = assets.write_ksplat(c, s_, wxyz, rgba)[0]
    else:
        rng = np.random.default_rng(5)
        data = assets.write_ply(c, np.log(s_), wxyz, rng.normal(0, 1, (n, 3)), rng.normal(0, 2, n))
    a = assets.SplatAsset(data, fmt, 0)
    arr = a.fill(want_scale_rotation=True)
    cam = surfel_cases._garden(160, 96)
    order = np.arange(n, dtype=np.uint32)
    host = SplatMesh(ctx, n, 0, render_mode_2d=True)
    host.build(arr["centers"], None, arr["rgba"], scales=arr["scales"], rotations=arr["rotations"])
    dev = SplatMesh(ctx, n, 0, render_mode_2d=True)
    a.upload_to(dev)
    seen = []
    for mesh in (host, dev):
        mesh.set_camera(cam)
        mesh.update_render_indexes(order, n)
        frame = mesh.render()[0]
        seen.append((frame, mesh.debug_records_2d(), mesh.debug_cull_planes()))
    (f0, (r0, q0, v0), (b0, x0, p0)), (f1, (r1, q1, v1), (b1, x1, p1)) = seen
    assert v0.sum() > 300 and f0.any()
    assert np.array_equal(b0, b1) and np.array_equal(x0, x1) and np.array_equal(p0, p1)
    assert np.array_equal(v0, v1) and np.array_equal(r0, r1) and np.array_equal(q0, q1) and np.array_equal(f0, f1)
    assert np.array_equal(b0, np.maximum(np.maximum(arr["scales"][:, 0] ** 2, arr["scales"][:, 1] ** 2), np.float32(1.0)))
    a.set_transform(np.eye(4))
    with pytest.raises(GsError) as e:
        a.upload_to(dev)
    assert e.value.status == L.GS_ERR_INVALID
    a.close()
    host.dispose()
    dev.dispose()


def test_what_a_surfel_mesh_refuses(ctx):
    h = L.C.c_void_p()
    with pytest.raises(GsError) as e:
        L.check(ctx.lib.gs_mesh_create(ctx.handle, 16, 0, L.GS_MESH_SURFEL | L.GS_MESH_COV_HALF, L.C.byref(h)))
    assert e.value.status == L.GS_ERR_INVALID and not h.value
    case, order, _ = surfel_cases.designed_case("quadrant_border")
    mesh, frame, _ = _draw(ctx, case, order)

    def refused(call):
        with pytest.raises(GsError) as err:
            call()
        assert err.value.status == L.GS_ERR_UNSUPPORTED and "SURFEL" in str(err.value)
    refused(lambda: mesh.set_draw_mode(rop8=True))
    refused(lambda: mesh.set_draw_mode(rop8=True, full=True))
    refused(lambda: mesh.rop8_window(0, 0, 8, 8))
    refused(lambda: mesh.surface(0, 0, 8, 8))
    refused(lambda: mesh.render(tile_rows=(0, 2)))
    refused(lambda: mesh.project(tile_rows=(1, 3)))
    group = L.C.c_void_p()
    L.check(ctx.lib.gs_group_create(ctx.handle, None, 1, 0, L.C.byref(group)))
    rows = (L.C.c_uint32 * 1)(0), (L.C.c_uint32 * 1)(64)
    mesh._cam.tile_row_begin = mesh._cam.tile_row_end = 0
    refused(lambda: L.check(ctx.lib.gs_group_render_gather(group, mesh.handle, L.C.byref(mesh._cam), None, None, 0, rows[0], rows[1], 0, None)))
    ctx.lib.gs_group_destroy(group)
    with pytest.raises(GsError):                                 # the 32-byte records do not exist
        mesh.debug_records()
    mesh.set_draw_mode(rop8=False)                               # the default mode is accepted, and the mesh still draws its frame
    again, _ = mesh.render()
    assert np.array_equal(again, frame) and frame.any()
    mesh.dispose()


def test_a_3d_mesh_beside_a_surfel_mesh_still_draws_its_frame(ctx):
    scene = helpers.small_scene(1500, 1, seed=11)
    cam = camera.demo_camera("garden", 200, 120)
    order = np.argsort(-(scene.centers.astype(np.float64) @ np.asarray(cam.sort_mvp(), np.float64).reshape(4, 4).T[2, :3]), kind="stable").astype(np.uint32)

    def frame_3d():
        mesh = SplatMesh(ctx, scene.count, 1)
        mesh.build(scene.centers, scene.cov, scene.rgba, scene.sh)
        mesh.set_camera(cam)
        mesh.update_render_indexes(order, scene.count)
        out = mesh.render()[0]
        return mesh, out
    alone, want = frame_3d()
    alone.dispose()
    case, s_order, _ = surfel_cases.frame_case("opaque")
    flat, _, _ = _draw(ctx, case, s_order)
    beside, got = frame_3d()
    flat.render()
    again = beside.render()[0]
    assert want.any() and np.array_equal(got, want) and np.array_equal(again, want)
    assert not (beside.view_share()["instance"] & 8)
    beside.dispose()
    flat.dispose()


# ---------------------------------------------------------------------------------------------------------------------------
# the engine against the reference's shader strings run on a real GL (tests/golden/surfel_gl_ref*.npz)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", surfel_cases.VERTEX_CASES)
def test_records_against_gl_transform_feedback(ctx, name):
    """max(4 d, the 3D check's figures) per field class, d = the recorded distance between the host model and GL; the factor 4
    covers llvmpipe's own association / FMA freedom on both sides of the model."""
    import test_surfel_ref as T
    case = surfel_cases.vertex_case(name)
    written, cap = T.gl_capture(name)
    mesh, _, _ = _draw(ctx, case, np.arange(2000, dtype=np.uint32))
    recs, rects, vis = mesh.debug_records_2d()
    mesh.dispose()
    assert written[vis].all()
    fl = recs[:, :17].view(np.float32)
    model = surfel_ref.vertex(case)
    inv = fl[:, 13:17].astype(np.float64)
    det = inv[:, 0] * inv[:, 3] - inv[:, 1] * inv[:, 2]
    with np.errstate(all="ignore"):                            # the basis back from its inverse: B = inverse(inverse basis)
        basis = np.stack([inv[:, 3] / det, -inv[:, 2] / det, -inv[:, 1] / det, inv[:, 0] / det], 1)
    engine = dict(tu=fl[:, 0:3], tv=fl[:, 3:6], tw=fl[:, 6:9], qc=fl[:, 9:11], c=fl[:, 11:13], basis=basis, c0=recs[:, 17], c1=recs[:, 18],
                  branch=model["branch"], ndcz=model["ndcz"])
    d = surfel_ref.gl_distances({k: a[written] for k, a in engine.items()}, cap, case["width"], case["height"])
    on = vis[written]
    for key, floor in T.FLOOR.items():
        if key == "ndcz":
            continue
        bound = max(4 * T.MANIFEST["vertex_distance"]["worst"][key], floor)
        worst = float(d[key][on].max())
        print(f"{name} {key}: engine to GL {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, key


@pytest.mark.parametrize("kind,name", [("frame", n) for n in surfel_cases.FRAME_CASES] +
                         [("designed", n) for n in surfel_cases.DESIGNED_CASES if n != "distance_reject"])
def test_frames_against_gl(ctx, kind, name):
    """Per value |engine - GL| <= |model fp32 - GL| + 1 step (the engine's single final rounding) on every non-ambiguous pixel,
    and the pixels no fragment reaches equal."""
    import test_surfel_ref as T
    case, order, dest = (surfel_cases.frame_case if kind == "frame" else surfel_cases.designed_case)(name)
    out = surfel_ref.render(case, order, **dest)
    gl = T.gl_frame(name).astype(int)
    mesh, got, _ = _draw(ctx, case, order, dest)
    mesh.dispose()
    clean = ~out["ambiguous"]
    excess = np.abs(got.astype(int) - gl) - np.abs(out["frame"].astype(int) - gl)
    print(f"{name}: engine to GL worst {int(np.abs(got.astype(int) - gl)[clean].max())}, model to GL worst "
          f"{int(np.abs(out['frame'].astype(int) - gl)[clean].max())}, worst excess {int(excess[clean].max())}")
    assert (excess[clean] <= 1).all()
    assert np.array_equal(got[~out["covered"]], gl[~out["covered"]].astype(np.uint8))
