"""-m gpu: gs_mesh_remove held to its definition - afterwards the mesh behaves, in every output, as a fresh mesh of the same
capacity and flags that received the survivors by the same uploads at their new positions.  Every scene is one upload (one Morton
run); layouts put run borders inside a storage block, on a block edge and in the last partial block.  Compared with the fresh
mesh: gs_mesh_debug_read 10 / 11 / 12 (every block of the capacity: the tail behind the survivors is a fresh mesh's too), a 64 x 64
frame from one shared host order in fp32 and both ROP8 modes, gs_mesh_surface and gs_mesh_bounds - byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from gaussiansplats3d_amd import Context, GsError, SplatMesh, camera
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER = (0.3, -1.7, 2.9)
LAYOUTS = [(300, 257, 443), (256, 512, 232)]
REMOVALS = {"first": [0], "middle": [1], "last": [2], "first_and_last": [0, 2]}
CONFIGS = {"sh0_fp32": dict(deg=0, half=False, u8=False), "sh2_fp16": dict(deg=2, half=True, u8=False), "sh2_fp32_u8": dict(deg=2, half=False, u8=True)}
MODES = [dict(rop8=False), dict(rop8=True), dict(rop8=True, full=True)]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def scene_data(n, deg, seed, u8=False):
    s = helpers.small_scene(n, deg, seed)
    sh = s.sh
    if u8 and deg:
        sh = np.random.default_rng(seed + 99).integers(0, 256, size=s.sh.shape, dtype=np.uint8)
    return s.centers, s.cov, s.rgba, sh


def new_mesh(ctx, capacity, cfg, **kw):
    m = SplatMesh(ctx, capacity, cfg["deg"], half_precision_covariances=cfg["half"], spherical_harmonics_8bit=cfg["u8"], **kw)
    if cfg["u8"] and not kw.get("dynamic_mode"):
        m.set_scenes(sh8_range=[(-1.0, 1.0)])
    m.set_camera(camera.demo_camera("garden", 64, 64))
    return m


def upload_runs(mesh, runs, scene_of=None):
    """each run is one upload, one behind the other"""
    at = 0
    for k, (c, cov, rgba, sh) in enumerate(runs):
        idx = None if scene_of is None else np.full(len(c), scene_of[k], np.uint32)
        mesh.build(c, cov, rgba, sh if sh.size else None, start=at, scene_indexes=idx)
        at += len(c)
    return at


def ranges_of(sizes, which):
    starts = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(starts[k]), int(sizes[k])) for k in which]


def planes(mesh, capacity):
    n, blocks = mesh.splat_count, (capacity + 255) // 256
    bound, pos, boxes = np.empty(n, np.float32), np.empty(n, np.uint32), np.empty((blocks, 8), np.float32)
    if n:
        L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 10, bound.ctypes.data, n))
        L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 12, pos.ctypes.data, n))
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 11, boxes.ctypes.data, blocks))
    return bound.tobytes(), boxes[:, :7].tobytes(), pos.tobytes()


def frames(mesh, order):
    """the frame in the three draw modes, then the surface planes of the last fp32 draw"""
    out = []
    for mode in MODES:
        mesh.set_draw_mode(**mode)
        mesh.update_render_indexes(order, len(order))
        out.append(mesh.render()[0].tobytes())
    mesh.set_draw_mode()
    mesh.render()
    ids, depth = mesh.surface(0, 0, 64, 64)
    return out + [ids.tobytes(), depth.tobytes()]


def same_as_fresh(edited, fresh, capacity, seed=5, with_planes=True):
    n = fresh.splat_count
    assert edited.splat_count == n
    if with_planes:
        for name, a, b in zip(("cov_bound", "block_box", "position"), planes(edited, capacity), planes(fresh, capacity)):
            assert a == b, name
    order = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    for name, a, b in zip(("fp32", "rop8", "rop8_full", "surface_ids", "surface_depth"), frames(edited, order), frames(fresh, order)):
        assert a == b, name
    if n:
        a, b = edited.bounds(0, n, CENTER), fresh.bounds(0, n, CENTER)
        assert a["count"] == b["count"] and a["min"].tobytes() == b["min"].tobytes() and a["max"].tobytes() == b["max"].tobytes()
        assert a["max_dist_sq"] == b["max_dist_sq"]
    assert np.frombuffer(frames(fresh, order)[0], np.uint8).any() or n == 0     # (the frame shows splats)


def removal_case(ctx, sizes, which, cfg, capacity=None, **kw):
    """builds the runs, removes the runs `which`, compares with the fresh mesh of the others; returns (edited, fresh, runs kept)"""
    capacity = capacity or sum(sizes) + 100
    runs = [scene_data(n, cfg["deg"], 40 + k, cfg["u8"]) for k, n in enumerate(sizes)]
    edited, fresh = new_mesh(ctx, capacity, cfg, **kw), new_mesh(ctx, capacity, cfg, **kw)
    upload_runs(edited, runs)
    edited.render()                                        # (a draw before: its state must not leak into the frames after)
    edited.remove(ranges_of(sizes, which))
    kept = [r for k, r in enumerate(runs) if k not in which]
    upload_runs(fresh, kept)
    same_as_fresh(edited, fresh, capacity)
    return edited, fresh, kept


@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
@pytest.mark.parametrize("which", list(REMOVALS), ids=list(REMOVALS))
@pytest.mark.parametrize("sizes", LAYOUTS, ids=["x".join(map(str, s)) for s in LAYOUTS])
def test_a_removal_leaves_a_fresh_mesh(ctx, sizes, which, cfg):
    edited, fresh, _ = removal_case(ctx, sizes, REMOVALS[which], CONFIGS[cfg])
    edited.dispose()
    fresh.dispose()


@pytest.mark.parametrize("sizes", [(1, 4096), (4096, 300)], ids=["shift_1_tail_4096", "shift_4096_tail_300"])
def test_source_and_destination_overlap(ctx, sizes):
    """a span far longer than its shift, and a shift longer than its span"""
    edited, fresh, _ = removal_case(ctx, sizes, [0], CONFIGS["sh2_fp16"])
    edited.dispose()
    fresh.dispose()


def test_uploads_after_a_removal(ctx):
    cfg, sizes = CONFIGS["sh2_fp16"], (300, 257, 443)
    edited, fresh, kept = removal_case(ctx, sizes, [1], cfg, capacity=1400)
    # a new run behind the survivors is a fresh run
    extra = scene_data(333, 2, 77)
    edited.build(*extra, start=743)
    fresh.build(*extra, start=743)
    same_as_fresh(edited, fresh, 1400)
    # ... which can go again on its own, and so can the run that moved
    edited.remove([(300, 443)])
    again = new_mesh(ctx, 1400, cfg)
    upload_runs(again, [kept[0], extra])
    same_as_fresh(edited, again, 1400)
    # new data into a survivor's shifted range keeps its slots: the frame is that of a fresh mesh of the same data
    other = scene_data(333, 2, 78)
    edited.build(*other, start=300)
    direct = new_mesh(ctx, 1400, cfg)
    upload_runs(direct, [kept[0], other])
    same_as_fresh(edited, direct, 1400, with_planes=False)
    pos = np.empty(633, np.uint32)
    L.check(edited.lib.gs_mesh_debug_read(edited.handle, 12, pos.ctypes.data, 633))
    assert planes(again, 1400)[2] == pos.tobytes()         # (the slots of the data before)
    for m in (edited, fresh, again, direct):
        m.dispose()


def test_a_dynamic_mesh_loses_its_middle_scene(ctx):
    cfg, sizes = CONFIGS["sh0_fp32"], (300, 257, 443)
    runs = [scene_data(n, 0, 60 + k) for k, n in enumerate(sizes)]
    t = [np.eye(4), np.eye(4), np.eye(4)]
    t[0][:3, 3], t[1][:3, 3], t[2][:3, 3] = (0.2, 0.0, 0.0), (0.0, 0.4, 0.0), (-0.3, 0.1, 0.2)
    t = [m.T.reshape(16) for m in t]                       # column-major
    edited, fresh = new_mesh(ctx, 1100, cfg, dynamic_mode=True), new_mesh(ctx, 1100, cfg, dynamic_mode=True)
    upload_runs(edited, runs, scene_of=[0, 1, 2])
    edited.set_scenes(transforms=t)
    edited.render()
    edited.remove([(300, 257)], scene_remap=[0, 0, 1])
    edited.set_scenes(transforms=[t[0], t[2]])
    upload_runs(fresh, [runs[0], runs[2]], scene_of=[0, 1])
    fresh.set_scenes(transforms=[t[0], t[2]])
    same_as_fresh(edited, fresh, 1100)
    moved = new_mesh(ctx, 1100, cfg, dynamic_mode=True)    # (the transforms matter: with scene 1's for the last run the frame differs)
    upload_runs(moved, [runs[0], runs[2]], scene_of=[0, 1])
    moved.set_scenes(transforms=[t[0], t[1]])
    order = np.arange(743, dtype=np.uint32)
    assert frames(moved, order)[0] != frames(fresh, order)[0]
    for m in (edited, fresh, moved):
        m.dispose()


def test_refusals_change_nothing(ctx):
    cfg, sizes = CONFIGS["sh0_fp32"], (300, 257, 443)
    runs = [scene_data(n, 0, 40 + k) for k, n in enumerate(sizes)]
    mesh = new_mesh(ctx, 1100, cfg)
    upload_runs(mesh, runs)
    order = np.random.default_rng(3).permutation(1000).astype(np.uint32)
    before = (planes(mesh, 1100), frames(mesh, order))
    bad = [([(310, 100)], None, "Morton run"), ([(0, 310)], None, "Morton run"), ([(557, 443), (0, 300)], None, "ascending"),
           ([(0, 300), (557, 0)], None, "empty"), ([(557, 544)], None, "max_splat_count"), ([(k, 1) for k in range(33)], None, "GS_MAX_SCENES"),
           ([(0, 300)], [0, 32], "scene_remap"), ([(0, 300)], list(range(33)), "scene_remap")]
    for ranges, remap, why in bad:
        with pytest.raises(GsError, match=why) as e:
            mesh.remove(ranges, scene_remap=remap)
        assert e.value.status == L.GS_ERR_INVALID
        assert mesh.splat_count == 1000
        assert (planes(mesh, 1100), frames(mesh, order)) == before, (ranges, remap)
    mesh.remove([])                                        # n_ranges == 0: nothing happens
    mesh.remove([(1000, 100)])                             # wholly behind the uploaded splats: nothing to remove
    ids_before = mesh.surface(0, 0, 64, 64)[0]             # (the last draw is still there)
    assert (planes(mesh, 1100), frames(mesh, order)) == before and ids_before.shape == (64, 64)
    mesh.dispose()
    # a mesh that keeps upload order accepts the range a Morton mesh refuses
    edited, fresh = new_mesh(ctx, 1100, cfg, keep_order=True), new_mesh(ctx, 1100, cfg, keep_order=True)
    upload_runs(edited, runs)
    edited.remove([(310, 100)])
    allc = [np.concatenate([r[k] for r in runs]) for k in range(3)]
    keep = np.r_[0:310, 410:1000]
    fresh.build(allc[0][keep], allc[1][keep], allc[2][keep], None)
    same_as_fresh(edited, fresh, 1100)
    edited.dispose()
    fresh.dispose()


def test_the_state_of_the_old_numbering_is_forgotten(ctx):
    cfg, sizes = CONFIGS["sh0_fp32"], (300, 257, 443)
    runs = [scene_data(n, 0, 40 + k) for k, n in enumerate(sizes)]
    edited, fresh = new_mesh(ctx, 1100, cfg), new_mesh(ctx, 1100, cfg)
    back = np.random.default_rng(8).integers(0, 256, size=(64, 64, 4), dtype=np.uint8)
    for m in (edited, fresh):
        m.set_destination(rgba=back)                       # a destination survives
    upload_runs(edited, runs)
    upload_runs(fresh, [runs[0], runs[2]])
    order = np.arange(743, dtype=np.uint32)
    edited.update_render_indexes(np.arange(1000, dtype=np.uint32), 1000)
    edited.render()
    edited.surface(0, 0, 64, 64)
    edited.project()                                       # a projection of 1000 splats is pending ...
    edited.remove([(300, 257)])
    with pytest.raises(GsError, match="no draw yet"):      # the last draw is gone
        edited.surface(0, 0, 64, 64)
    with pytest.raises(GsError, match="no draw"):
        edited.rop8_window(0, 0, 8, 8)
    with pytest.raises(GsError, match="no draw"):
        edited.debug_records(10)
    with pytest.raises(GsError, match="exceeds the uploaded"):
        edited.update_render_indexes(np.arange(1000, dtype=np.uint32), 1000)
        edited.render()
    edited.update_render_indexes(order, 743)
    fresh.update_render_indexes(order, 743)
    a, b = edited.render()[0], fresh.render()[0]           # ... and is dropped: this draw projects the 743 that are left
    assert a.tobytes() == b.tobytes() and (a != back).any()
    stats_a, stats_b = edited.last_stats(), fresh.last_stats()
    assert stats_a.visible_splats == stats_b.visible_splats and stats_a.tile_entries == stats_b.tile_entries
    same_as_fresh(edited, fresh, 1100)
    edited.dispose()
    fresh.dispose()


def test_under_poisoned_allocations_in_a_child_process():
    """the same comparison with every new allocation holding 0xFF: nothing may depend on what the allocator left"""
    env = dict(os.environ, GSPLAT_POISON_ALLOC="0xFF")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "tools", "remove_child.py")], env=env, text=True, timeout=120)
    assert out.strip().splitlines()[-1] == "remove_child: ok"
