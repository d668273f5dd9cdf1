"""-m gpu: k_bin_emit's live units (csrc/tile_bin.hip, csrc/draw_plan.hpp) - only batches that hold a splat are dealt, and the next
unit's loads are issued before this one is expanded - against the host model of the draw order (bin_lists_ref.py), with the scenes,
the draw and the comparison of test_gpu_bin_lists.py.  Exact: every range, every entry, the statistics.

The dealing has no switch, so the model is what holds it; each case asserts from the MODEL's data that the draw has the shape it is
named for.  (A truncated draw and a draw that is redone after an overflow - the `first entry slot >= D` rule, which now sits where
a unit is loaded - are held by test_gpu_bin_lists.py's two overflow cases; one more shape of the redone draw is here.)
Frames are 256 x 256 px."""
import numpy as np
import pytest

import bin_lists_ref as ref
import test_gpu_bin_lists as bl
from gaussiansplats3d_amd import Context, camera

pytestmark = pytest.mark.gpu
W = H = 256
BATCH, MAX_GRID, EMIT_OWN, SORT_TILE = 256, 2048, 16, 4096
SPREAD = (100.0, 100.0)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def cam_of():
    return camera.demo_camera("garden", W, H)


def order_of_walk(walk):
    """The render list whose near -> far walk is `walk` (the binner walks the list from its end)."""
    return np.ascontiguousarray(np.asarray(walk, dtype=np.uint32)[::-1])


def live_units_of(want, R):
    """(per, survivors per slice, live batches) of the draw, from the model's walk positions."""
    batches = -(-R // BATCH)
    grid = min(max(batches, 1), MAX_GRID)
    per = -(-batches // grid)
    per_slice = np.bincount(want.walk_q // (per * BATCH), minlength=grid)
    return per, per_slice, int((-(-per_slice // BATCH)).sum())


def test_one_batch_per_slice_and_most_workgroups_without_a_unit(ctx):
    """70 001 list positions: 274 slices of one batch.  What is visible lies together in the walk, so a handful of slices is live and
    most of the emit's workgroups find no unit at all."""
    cam = cam_of()
    rng = np.random.default_rng(5)
    n, seen = 70_001, 3000
    scene = bl.scene_of([bl.behind(cam, n - seen, rng), bl.placed(cam, seen, rng.uniform(2.0, 40.0, seen), rng, spread_px=SPREAD)], 5)
    walk = np.concatenate([np.arange(0, 30_000), np.arange(n - seen, n), np.arange(30_000, n - seen)])
    mesh = bl.build_mesh(ctx, scene)
    want, _ = bl.check(mesh, cam, order_of_walk(walk), n, bl.draw(mesh, cam, order_of_walk(walk), n))
    per, per_slice, live = live_units_of(want, n)
    assert per == 1 and per_slice.shape[0] == 274 and want.walk.shape[0] > seen // 2
    assert 0 < live == (per_slice > 0).sum() < 274 // 4 and per_slice[0] == 0 and per_slice[-1] == 0
    mesh.dispose()


def test_empty_leading_slices_then_slices_of_256_and_257_survivors(ctx):
    """600 000 list positions: slices of two batches.  The nearest ten slices hold nothing visible (their words share the first
    unit 0), then come slices with exactly 256 survivors (one full batch, the second dead), 257 (a second batch of one splat), 512
    and 1; the rest of the walk is mixed, and the slices behind the end of the list are empty again."""
    cam = cam_of()
    rng = np.random.default_rng(6)
    n, marks, small = 600_000, 2000, 20_000
    scene = bl.scene_of([bl.behind(cam, n - marks - small, rng), bl.placed(cam, small, rng.uniform(1.0, 12.0, small), rng, spread_px=SPREAD),
                         bl.placed(cam, marks, 30.0, rng, spread_px=SPREAD)], 6)
    hidden, mark = iter(range(0, n - marks - small)), iter(range(n - marks, n))
    take = lambda it, k: [next(it) for _ in range(k)]
    S = 2 * BATCH
    head = take(hidden, 10 * S)
    for k in (256, 257, 512, 1):
        head += take(mark, k) + take(hidden, S - k)
    used = np.zeros(n, dtype=bool)
    used[head] = True
    rest = np.random.default_rng(7).permutation(np.nonzero(~used)[0])
    walk = np.concatenate([np.asarray(head), rest])
    order = order_of_walk(walk)
    mesh = bl.build_mesh(ctx, scene)
    want, _ = bl.check(mesh, cam, order, n, bl.draw(mesh, cam, order, n))
    per, per_slice, live = live_units_of(want, n)
    assert per == 2 and per_slice[:14].tolist() == [0] * 10 + [256, 257, 512, 1]
    last = (n - 1) // S                                     # the grid is at its cap: the slices behind the list's end are empty too
    assert per_slice.shape[0] == MAX_GRID and (per_slice[14:last] > 0).all() and (per_slice[last + 1:] == 0).all()
    assert live == int((-(-per_slice // BATCH)).sum()) < 2 * last
    mesh.dispose()


def test_whole_frame_splats_share_a_batch_with_small_ones(ctx, monkeypatch):
    """64 lists of 32 px: a splat over the whole frame has 64 entries, 16 from its lane and 48 from the wave.  The 200 of them are the
    nearest splats, so one batch's entries span several of the entry sort's 4096-entry tiles."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = cam_of()
    rng = np.random.default_rng(8)
    scene = bl.scene_of([bl.placed(cam, 1500, rng.uniform(2.0, 20.0, 1500), rng, spread_px=SPREAD),
                         bl.placed(cam, 200, 1500.0, rng, spread_px=(20.0, 20.0), depth=(0.8, 1.5))], 8)
    order = bl.draw_order(scene, cam, permuted=False)
    mesh = bl.build_mesh(ctx, scene)
    want, _ = bl.check(mesh, cam, order, scene.count, bl.draw(mesh, cam, order, scene.count))
    assert want.ranges.shape[0] == 64 and (want.runs == 64).sum() >= 150 and (want.runs <= EMIT_OWN).sum() > 500
    per_batch = np.bincount(want.walk_q // BATCH, weights=want.runs)
    assert per_batch.max() > 2 * SORT_TILE
    first = want.walk_q // BATCH == np.argmax(per_batch)
    assert (want.runs[first] == 64).any() and (want.runs[first] <= EMIT_OWN).any()
    mesh.dispose()


@pytest.fixture(scope="module")
def one_list_mesh(ctx):
    """A mesh whose frame is ONE list of 256 px: every visible splat is one entry.  (mesh, cam, scene, indexes of the visible)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("GSPLAT_LIST_SHIFT", "4")                     # read when the mesh is created
    cam = cam_of()
    scene = bl.cloud(cam, 30_000, seed=9, huge=3)
    mesh = bl.build_mesh(ctx, scene)
    mp.undo()
    order = bl.draw_order(scene, cam, permuted=True, seed=9)
    stats = bl.draw(mesh, cam, order, scene.count)
    assert stats.list_bin_px == 256
    _, _, vis = mesh.debug_records()
    seen = order[vis[order]]
    assert seen.shape[0] > SORT_TILE + 1
    yield mesh, cam, scene, seen
    mesh.dispose()


@pytest.mark.parametrize("total", [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_entry_totals_around_one_sort_tile(one_list_mesh, total):
    mesh, cam, scene, seen = one_list_mesh
    order = np.ascontiguousarray(seen[:total])
    want, _ = bl.check(mesh, cam, order, total, bl.draw(mesh, cam, order, total))
    assert want.entries.shape[0] == total and want.ranges.tolist() == [[0, total]]


def test_a_draw_in_which_nothing_is_visible(ctx):
    cam = cam_of()
    scene = bl.scene_of([bl.behind(cam, 3000, np.random.default_rng(10))], 10)
    order = np.arange(scene.count, dtype=np.uint32)
    mesh = bl.build_mesh(ctx, scene)
    want, (vis, *_) = bl.check(mesh, cam, order, scene.count, bl.draw(mesh, cam, order, scene.count))
    ranges, entries, _ = mesh.bin_lists()
    assert not vis.any() and entries.shape[0] == 0 and (ranges == ref.UNTOUCHED).all()
    mesh.dispose()


def test_a_strip_whose_first_list_row_is_not_row_zero(ctx, monkeypatch):
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = cam_of()
    scene = bl.cloud(cam, 6000, seed=12)
    order = bl.draw_order(scene, cam, permuted=True, seed=12)
    rows = (5, 12)                                          # tile rows: list-bin rows 2 .. 5
    mesh = bl.build_mesh(ctx, scene)
    stats = bl.draw(mesh, cam, order, scene.count, tile_rows=rows)
    want, (*_, row_begin) = bl.check(mesh, cam, order, scene.count, stats, tile_rows=rows)
    assert row_begin == 2 and want.ranges.shape[0] == 8 * 4 and want.entries.shape[0] > 500
    mesh.dispose()


def test_a_draw_that_overflows_between_two_units_is_redone(ctx, monkeypatch):
    """Room for 4096 entries where the nearest batch alone needs more: every later unit's first entry slot is past the room, and the
    synchronous draw is repeated with grown buffers."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = cam_of()
    scene = bl.cloud(cam, 8000, seed=14, huge=250)
    order = bl.draw_order(scene, cam, permuted=False)
    mesh = bl.build_mesh(ctx, scene)
    mesh.debug_set_entry_capacity(SORT_TILE)
    stats = bl.draw(mesh, cam, order, scene.count)
    want, _ = bl.check(mesh, cam, order, scene.count, stats)
    assert stats.overflowed == 1 and want.entries.shape[0] > 3 * SORT_TILE
    mesh.dispose()


def test_a_large_draw_then_a_small_one_on_the_same_mesh(ctx):
    cam = cam_of()
    scene = bl.cloud(cam, 20_000, seed=15)
    order = bl.draw_order(scene, cam, permuted=True, seed=15)
    mesh = bl.build_mesh(ctx, scene)
    big, _ = bl.check(mesh, cam, order, scene.count, bl.draw(mesh, cam, order, scene.count))
    R = 300
    small, _ = bl.check(mesh, cam, order, R, bl.draw(mesh, cam, order, R))
    assert big.walk.shape[0] > 20 * small.walk.shape[0] > 0 and -(-scene.count // BATCH) > 64
    mesh.dispose()


def test_fresh_buffers_that_hold_no_zeros(monkeypatch):
    """Under GSPLAT_POISON_ALLOC every new allocation holds 0xFF: a slice sum, a count or a word read before it was written shows."""
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", "0xFF")       # (read at every allocation: stays set for the whole test)
    own = Context(0)
    try:
        cam = cam_of()
        scene = bl.cloud(cam, 5000, seed=16)
        order = bl.draw_order(scene, cam, permuted=True, seed=16)
        mesh = bl.build_mesh(own, scene)
        want, _ = bl.check(mesh, cam, order, scene.count, bl.draw(mesh, cam, order, scene.count))
        assert want.entries.shape[0] > 5000
    finally:
        own.close()
