"""-m gpu: gs_mesh_reorder held to its definition - afterwards the mesh behaves, in every output, as a fresh mesh of the same
capacity and flags in which the folded range arrived by ONE upload and every other range by the uploads it did arrive by.
Compared with that fresh mesh as tests/test_gpu_mesh_remove.py compares: gs_mesh_debug_read 10 / 11 / 12 over every block of the
capacity, a 64 x 64 frame from one shared host order in fp32 and both ROP8 modes, gs_mesh_surface and gs_mesh_bounds - byte for
byte.  Read 12 (the storage position of every splat) is also held to morton_ref's prediction, and before every fold the test
asserts that read 12 DIFFERS from the fresh mesh's: pieces that already gave the final order would show nothing."""
import types

import numpy as np
import pytest

import helpers
import morton_ref
from gaussiansplats3d_amd import Context, GsError, SplatMesh, assets, camera, create_sort_worker
from gaussiansplats3d_amd import _lib as L
from test_gpu_asset_upload import synthetic_splats
from test_gpu_mesh_remove import CONFIGS, frames, new_mesh, planes, same_as_fresh, scene_data, upload_runs
from test_gpu_sorter_remove import Trio, upload as upload_centres

pytestmark = pytest.mark.gpu
LAYOUTS = [(300, 257, 443), (256, 512, 232)]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def joined(runs):
    """the runs as ONE upload"""
    return tuple(np.concatenate([r[k] for r in runs]) for k in range(4))


def position(mesh):
    pos = np.empty(mesh.splat_count, np.uint32)
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 12, pos.ctypes.data, mesh.splat_count))
    return pos


def fold_case(ctx, runs, a, b, cfg, capacity=None, reupload=None):
    """uploads the runs one by one, folds runs [a, b) and compares with the fresh mesh that received them by one upload;
    reupload = (start, data): new data for splats inside the range before the fold - they keep their slots until the fold, which
    orders the range by the centres it holds then.  Returns (edited, fresh)"""
    sizes = [len(r[0]) for r in runs]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    capacity = capacity or int(starts[-1]) + 100
    frm, count = int(starts[a]), int(starts[b] - starts[a])
    edited, fresh = new_mesh(ctx, capacity, cfg), new_mesh(ctx, capacity, cfg)
    upload_runs(edited, runs)
    one = joined(runs[a:b])
    if reupload:
        at, data = reupload
        edited.build(*data, start=at)
        for k in range(4):
            one[k][at - frm:at - frm + len(data[0])] = data[k]
    upload_runs(fresh, runs[:a] + [one] + runs[b:])
    edited.render()                                        # (a draw before: its state must not leak into the frames after)
    before, want = position(edited), position(fresh)
    assert before.tobytes() != want.tobytes(), "the pieces already gave the final order: the case shows nothing"
    edited.reorder(frm, count)
    same_as_fresh(edited, fresh, capacity)
    got = position(edited)
    assert np.array_equal(got[frm:frm + count], morton_ref.positions(one[0], frm))
    assert np.array_equal(got[:frm], before[:frm]) and np.array_equal(got[frm + count:], before[frm + count:])   # the neighbours stay
    return edited, fresh


def runs_of(sizes, cfg, seed=40):
    return [scene_data(n, cfg["deg"], seed + k, cfg["u8"]) for k, n in enumerate(sizes)]


def dispose(*meshes):
    for m in meshes:
        m.dispose()


@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
@pytest.mark.parametrize("sizes", LAYOUTS, ids=["x".join(map(str, s)) for s in LAYOUTS])
def test_a_whole_mesh_folds_into_one_run(ctx, sizes, cfg):
    dispose(*fold_case(ctx, runs_of(sizes, CONFIGS[cfg]), 0, 3, CONFIGS[cfg]))


@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
@pytest.mark.parametrize("sizes", LAYOUTS, ids=["x".join(map(str, s)) for s in LAYOUTS])
def test_the_middle_two_of_four_runs(ctx, sizes, cfg):
    """the range begins inside a storage block or on a block edge and ends inside the block the last run begins in; the first
    and the last run stay where they are"""
    dispose(*fold_case(ctx, runs_of(sizes + (130,), CONFIGS[cfg]), 1, 3, CONFIGS[cfg]))


def test_forty_small_runs(ctx):
    sizes = np.random.default_rng(17).integers(1, 71, size=40).tolist()
    assert min(sizes) == 1 and max(sizes) == 70
    dispose(*fold_case(ctx, runs_of(sizes, CONFIGS["sh2_fp16"]), 0, 40, CONFIGS["sh2_fp16"]))


@pytest.mark.parametrize("sizes", [(1, 4096), (4095, 2)], ids=["1_4096", "4095_2"])
def test_across_the_radix_tile(ctx, sizes):
    dispose(*fold_case(ctx, runs_of(sizes, CONFIGS["sh2_fp16"]), 0, 2, CONFIGS["sh2_fp16"]))


def test_ties_across_a_run_border_keep_the_original_index_order(ctx):
    """run 2 repeats every centre of run 0 bit for bit and one axis has extent 0: every key of run 0 ties with a key 557 later"""
    cfg = CONFIGS["sh0_fp32"]
    runs = [list(r) for r in runs_of((300, 257, 300), cfg)]
    level = runs[0][0][0, 1]
    for r in runs:
        r[0] = r[0].copy()
        r[0][:, 1] = level                                 # extent 0 on y
    runs[2][0] = runs[0][0].copy()
    runs = [tuple(r) for r in runs]
    c = joined(runs)[0]
    keys, pos = morton_ref.keys(c), morton_ref.positions(c)
    assert np.array_equal(keys[:300], keys[557:]) and np.array_equal(c[:300].view(np.uint32), c[557:].view(np.uint32))
    assert ((keys >> 1) & 1).max() == 0 and (morton_ref.bounds(c)[0][1], morton_ref.bounds(c)[1][1]) == (level, level)
    assert (pos[:300] < pos[557:]).all()                   # the model: the lower original index first
    assert len(np.unique(keys)) < len(keys) - 200
    edited, fresh = fold_case(ctx, runs, 0, 3, cfg)
    got = position(edited)
    assert (got[:300] < got[557:]).all() and np.array_equal(got, pos)
    dispose(edited, fresh)


def test_a_nan_and_an_infinite_centre(ctx):
    """NaN never moves a bound (its key is 0); an infinite value does (the axis' extent is infinite: every key bit of it is 0)"""
    cfg = CONFIGS["sh2_fp16"]
    runs = [list(r) for r in runs_of((300, 257, 443), cfg)]
    runs[0][0], runs[1][0] = runs[0][0].copy(), runs[1][0].copy()
    runs[0][0][17, 2] = np.nan
    runs[1][0][100, 0] = np.inf
    runs = [tuple(r) for r in runs]
    c = joined(runs)[0]
    mn, mx = morton_ref.bounds(c)
    assert mx[0] == np.inf and np.isfinite(mn).all() and np.isfinite(mx[1:]).all()
    assert (morton_ref.keys(c) & 1).max() == 0 and (morton_ref.keys(c) >> 2 & 1).max() == 1
    dispose(*fold_case(ctx, runs, 0, 3, cfg))


# ------------------------------------------------------------------------------------------------ assets in pieces
def asset_files():
    c, s, q, rgba, sh = synthetic_splats(3000, 1, 9)
    unit, logit = rgba / 255.0, np.log((rgba[:, 3] + 0.5) / (255.5 - rgba[:, 3]))
    f_dc = (unit[:, :3] - 0.5) / 0.28209479177387814
    return {"ksplat": (assets.write_ksplat(c, s, q, rgba, sh, 1, 1, block_size=2.0, bucket_size=256, sh_range=(-1.2, 1.3))[0], "ksplat"),
            "ply": (assets.write_ply(c, np.log(s), q, f_dc, logit, sh), "ply")}


@pytest.mark.parametrize("kind", ["ksplat", "ply"])
def test_an_asset_uploaded_in_pieces_folds_to_one_upload(ctx, kind):
    """SplatAsset.upload_to in pieces of 1 057 splats, then one fold == one upload_to of the whole; the bounds of every run are
    reduced on the device on both sides"""
    data, fmt = asset_files()[kind]
    asset = assets.SplatAsset(data, fmt, 1)
    n = asset.info.splat_count
    assert n == 3000
    cfg = dict(deg=1, half=False, u8=asset.info.sh_level == 2)
    edited, fresh = new_mesh(ctx, n + 50, cfg), new_mesh(ctx, n + 50, cfg)
    for at in range(0, n, 1057):
        asset.upload_to(edited, at, at, min(1057, n - at), 1)
    asset.upload_to(fresh, 0, 0, n, 1)
    assert position(edited).tobytes() != position(fresh).tobytes()
    edited.render()
    edited.reorder()
    same_as_fresh(edited, fresh, n + 50)
    dispose(edited, fresh)
    asset.close()


# ------------------------------------------------------------------------------------------------ state
def test_uploads_and_a_removal_around_a_fold(ctx):
    cfg, sizes = CONFIGS["sh2_fp16"], (300, 257, 443)
    runs = runs_of(sizes, cfg)
    other = scene_data(120, 2, 91)
    edited, fresh = fold_case(ctx, runs, 0, 2, cfg, capacity=1500, reupload=(250, other))   # across the border of runs 0 and 1
    edited.reorder(0, 557)                                 # a second fold has nothing to do: the last draw still answers
    edited.render()
    ids = edited.surface(0, 0, 64, 64)[0]
    edited.reorder(0, 557)
    assert np.array_equal(edited.surface(0, 0, 64, 64)[0], ids)
    extra = scene_data(333, 2, 77)                         # an appended upload is a run of its own on both
    for m in (edited, fresh):
        m.build(*extra, start=1000)
    same_as_fresh(edited, fresh, 1500)
    for m in (edited, fresh):                              # the neighbouring scene goes; the folded run is a run like any other
        m.remove([(557, 443)])
    same_as_fresh(edited, fresh, 1500)
    with pytest.raises(GsError, match="Morton run"):
        edited.remove([(300, 257)])                        # the old border at 300 is no border any more
    edited.reorder()                                       # ... and what is left folds again
    again = new_mesh(ctx, 1500, cfg)
    data = [np.concatenate([joined(runs[:2])[k], extra[k]]) for k in range(4)]
    for k in range(4):
        data[k][250:370] = other[k]
    again.build(*data)
    same_as_fresh(edited, again, 1500)
    dispose(edited, fresh, again)


def test_the_state_of_the_old_order_is_forgotten(ctx):
    cfg, sizes = CONFIGS["sh0_fp32"], (300, 257, 443)
    runs = runs_of(sizes, cfg)
    edited, fresh = new_mesh(ctx, 1100, cfg), new_mesh(ctx, 1100, cfg)
    back = np.random.default_rng(8).integers(0, 256, size=(64, 64, 4), dtype=np.uint8)
    for m in (edited, fresh):
        m.set_destination(rgba=back)                       # a destination survives
    upload_runs(edited, runs)
    upload_runs(fresh, [joined(runs)])
    order = np.random.default_rng(4).permutation(1000).astype(np.uint32)
    edited.update_render_indexes(order, 1000)
    edited.render()
    edited.surface(0, 0, 64, 64)
    edited.project()                                       # a projection of the old layout is pending ...
    edited.reorder()
    with pytest.raises(GsError, match="no draw yet"):      # the last draw is gone
        edited.surface(0, 0, 64, 64)
    with pytest.raises(GsError, match="no draw"):
        edited.rop8_window(0, 0, 8, 8)
    with pytest.raises(GsError, match="no draw"):
        edited.debug_records(10)
    fresh.update_render_indexes(order, 1000)
    a, b = edited.render()[0], fresh.render()[0]           # ... and is dropped: this draw projects the new layout
    assert a.tobytes() == b.tobytes() and (a != back).any()
    stats_a, stats_b = edited.last_stats(), fresh.last_stats()
    assert stats_a.visible_splats == stats_b.visible_splats and stats_a.tile_entries == stats_b.tile_entries
    same_as_fresh(edited, fresh, 1100)
    dispose(edited, fresh)


def bound_trio(ctx, centres, cam, seeds, one_upload):
    """test_gpu_sorter_remove's Trio - a mesh and a sorter bound to it - whose mesh receives the scenes by one upload or one each"""
    t = types.SimpleNamespace(cam=cam, mvp=cam.sort_mvp(), mesh=SplatMesh(ctx, 1100, 0), worker=create_sort_worker(ctx, 1100), tree=None)
    parts = [helpers.small_scene(len(c), 0, seeds[k]) for k, c in enumerate(centres)]
    data = [(c, p.cov, p.rgba) for c, p in zip(centres, parts)]
    if one_upload:
        data = [tuple(np.concatenate([d[k] for d in data]) for k in range(3))]
    at = 0
    for c, cov, rgba in data:
        t.mesh.build(c, cov, rgba, None, start=at)
        at += len(c)
    upload_centres(t.worker, centres, [0] * len(centres), True)
    t.mesh.set_camera(cam)
    t.mesh.use_sorter_result(t.worker, at)                 # binds
    t.n = at
    return t


def test_a_bound_sorter_with_the_visibility_cull(ctx):
    cam = camera.demo_camera("garden", 64, 64)
    centres = [helpers.small_scene(n, 0, 21 + k).centers for k, n in enumerate((300, 257, 443))]
    edited, fresh = bound_trio(ctx, centres, cam, (21, 22, 23), False), bound_trio(ctx, centres, cam, (21, 22, 23), True)
    try:
        assert position(edited.mesh).tobytes() != position(fresh.mesh).tobytes()
        kept_before, frame_before = Trio.culled_frame(edited)   # project, sort, draw: resident result, derived mask, position map
        edited.mesh.reorder()
        with pytest.raises(GsError, match="no device-resident result"):   # as after gs_mesh_remove
            edited.mesh.render()
        with pytest.raises(GsError, match="no sort has run"):
            edited.worker.debug_read(2, 10)
        kept, frame = Trio.culled_frame(edited)
        kept_fresh, frame_fresh = Trio.culled_frame(fresh)
        assert 0 < len(kept) < 1000 and frame.any()
        assert np.array_equal(kept, kept_fresh) and frame.tobytes() == frame_fresh.tobytes()
        assert np.array_equal(kept, kept_before) and frame.tobytes() == frame_before.tobytes()   # (the picture never depended on the layout)
        assert position(edited.mesh).tobytes() == position(fresh.mesh).tobytes()
    finally:
        Trio.close(edited)
        Trio.close(fresh)


# ------------------------------------------------------------------------------------------------ refusals and no-ops
def test_refusals_change_nothing(ctx):
    cfg = CONFIGS["sh0_fp32"]
    runs = runs_of((300, 257, 443), cfg)
    mesh = new_mesh(ctx, 1400, cfg)
    upload_runs(mesh, runs[:2])
    mesh.build(*runs[2][:3], None, start=657)              # [557, 657) was never uploaded
    order = np.random.default_rng(3).permutation(1100).astype(np.uint32)
    before = (planes(mesh, 1400), frames(mesh, order))
    for frm, count, why in [(10, 547, "Morton run"), (0, 400, "Morton run"), (0, 1100, "never uploaded"), (557, 100, "never uploaded"),
                            (0, 1101, "exceeds the uploaded"), (1100, 5, "exceeds the uploaded")]:
        with pytest.raises(GsError, match=why) as e:
            mesh.reorder(frm, count)
        assert e.value.status == L.GS_ERR_INVALID and mesh.splat_count == 1100
        assert (planes(mesh, 1400), frames(mesh, order)) == before, (frm, count)
    mesh.dispose()


def test_nothing_to_do_keeps_the_last_draw(ctx):
    cfg = CONFIGS["sh0_fp32"]
    runs = runs_of((300, 257, 443), cfg)
    order = np.random.default_rng(3).permutation(1000).astype(np.uint32)
    for keep_order, calls in ((False, [(300, 257), (0, 0), (557, 443)]), (True, [(0, 1000), (10, 5)])):
        mesh = new_mesh(ctx, 1100, cfg, keep_order=keep_order)
        upload_runs(mesh, runs)
        before = (planes(mesh, 1100), frames(mesh, order))
        ids = mesh.surface(0, 0, 64, 64)[0]
        for frm, count in calls:
            mesh.reorder(frm, count)                       # GS_OK
            assert np.array_equal(mesh.surface(0, 0, 64, 64)[0], ids)      # the last draw still answers
        assert (planes(mesh, 1100), frames(mesh, order)) == before
        mesh.dispose()
