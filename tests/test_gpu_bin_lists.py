"""-m gpu: the binner's entry lists (csrc/tile_bin.hip: k_bin_count, k_bin_emit, the entry sort) against the host model of
the draw order (bin_lists_ref.py).  Exact: np.array_equal on every range and on every entry, no tolerance anywhere.

Every case draws once, reads the vertex stage's own outputs (gs_mesh_debug_read what = 1 / 3 / 9) as the model's input and the
lists (what = 2 / 8) as the result, and asserts from the MODEL's data that the mechanism it is named for is really exercised.
"""
import numpy as np
import pytest

import bin_lists_ref as ref
import helpers
import oracle
from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
W, H = 1000, 562                      # 62.5 x 35.1 tiles: the last tile, list bin and blend bin of both axes are partial
NONE = 0xFFFFFFFF
BATCH, MAX_GRID = 256, 2048           # BIN_THREADS and BIN_MAX_BLOCKS of tile_bin.hip


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# -- scenes ---------------------------------------------------------------------------------------------------------------------
def placed(cam, count, radius_px, rng, spread_px=(300.0, 150.0), depth=(2.0, 6.0)):
    """Hand-placed isotropic splats in front of `cam`: centres within +-spread_px of the screen centre, about radius_px (sqrt(8)
    standard deviations) on screen.  Returns (centers, cov)."""
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    right, up, fwd = mw[0:3], mw[4:7], -mw[8:11]
    focal = cam.focal()[1]
    d = rng.uniform(depth[0], depth[1], size=(count, 1))
    off = rng.uniform(-1.0, 1.0, size=(count, 2)) * np.asarray(spread_px) * d / focal
    centers = cam.position + fwd * d + right * off[:, :1] + up * off[:, 1:]
    s = (np.broadcast_to(np.asarray(radius_px, dtype=np.float64), (count,)) * d[:, 0] / (np.sqrt(8.0) * focal)) ** 2
    zero = np.zeros(count)
    return centers.astype(np.float32), np.stack([s, zero, zero, s, zero, s], axis=1).astype(np.float32)


def behind(cam, count, rng):
    """Splats strictly behind the eye: they draw nothing."""
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    centers = cam.position + mw[8:11] * rng.uniform(0.5, 9.0, size=(count, 1)) + rng.normal(size=(count, 3)) * 0.2
    return centers.astype(np.float32), np.tile(np.array([[1e-4, 0, 0, 1e-4, 0, 1e-4]], np.float32), (count, 1))


def scene_of(parts, seed):
    centers = np.concatenate([p[0] for p in parts]).astype(np.float32)
    cov = np.concatenate([p[1] for p in parts]).astype(np.float32)
    rgba = np.random.default_rng(seed).integers(1, 256, size=(centers.shape[0], 4), dtype=np.uint8)
    return scenes.SplatScene(centers, cov, rgba, np.zeros((centers.shape[0], 0), np.float16), 0)


def cloud(cam, n, seed, huge=6, markers=0, scale=0.06):
    """helpers.small_scene + `huge` near splats that cover the whole frame (the screen-size cap makes them 1024 px) + `markers`
    splats of ~30 px that are certainly on screen.  The markers are the LAST indexes, the huge ones come before them."""
    rng = np.random.default_rng(seed)
    base = helpers.small_scene(n, 0, seed, scale=scale)
    return scene_of([(base.centers, base.cov), placed(cam, huge, 1500.0, rng, depth=(0.8, 1.5)), placed(cam, markers, 30.0, rng)], seed)


def build_mesh(ctx, scene, **kw):
    mesh = SplatMesh(ctx, scene.count, 0, False, **kw)
    mesh.build(scene.centers, scene.cov, scene.rgba, None)
    return mesh


def depth_order(scene, cam):
    return oracle.sort_indexes(np.arange(scene.count, dtype=np.uint32), util.integer_centers(scene.centers), cam.sort_mvp())


def draw_order(scene, cam, permuted, seed=0):
    """Half of the cases draw in true depth order; the other half in a seeded permutation: the binner honours whatever list it is
    given, and a permutation makes an order bug show in every list."""
    if permuted:
        return np.random.default_rng(1000 + seed).permutation(scene.count).astype(np.uint32)
    return depth_order(scene, cam)


# -- the comparison -------------------------------------------------------------------------------------------------------------
def grid_of(cam, list_px, tile_rows=None):
    """(list_shift, lists_x, first list-bin row, list-bin rows) of a draw: gs_render_stats.list_bin_px and the strip's tile rows."""
    rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
    r0, r1 = (0, rows_total) if tile_rows is None else tile_rows
    y0, y1 = r0 * L.GS_TILE, min(r1 * L.GS_TILE, cam.height)
    b0 = y0 // list_px
    b1 = (y1 + list_px - 1) // list_px if y1 > y0 else b0
    return int(list_px // L.GS_TILE).bit_length() - 1, (cam.width + list_px - 1) // list_px, b0, b1 - b0


def first_difference(ranges, entries, want, lists_x, row_begin):
    """Which list is wrong, and how: the message of a failing comparison."""
    for i in range(max(ranges.shape[0], want.ranges.shape[0])):
        if i >= ranges.shape[0] or i >= want.ranges.shape[0]:
            return f"the draw has {ranges.shape[0]} lists, the model {want.ranges.shape[0]}"
        (b, e), (wb, we) = (int(v) for v in ranges[i]), (int(v) for v in want.ranges[i])
        mine = entries[b:e] if e > b and e <= entries.shape[0] else entries[:0]
        theirs = want.entries[wb:we] if we > wb else want.entries[:0]
        if (b, e) != (wb, we) or not np.array_equal(mine, theirs):
            k = next((j for j in range(min(len(mine), len(theirs))) if mine[j] != theirs[j]), min(len(mine), len(theirs)))
            return (f"list {i} (bin x {i % lists_x}, y {row_begin + i // lists_x}): range ({b}, {e}) vs the model's ({wb}, {we}); "
                    f"first differing entry {k} of {len(mine)} / {len(theirs)}: "
                    f"{mine[k:k + 4].tolist()} vs {theirs[k:k + 4].tolist()}")
    return "the lists agree"


def model_of(mesh, cam, order, R, list_px, tile_rows=None):
    ranges, entries, slots = mesh.bin_lists(tile_rows, list_bin_px=list_px)
    _, rects, vis = mesh.debug_records()
    shift, lists_x, row_begin, rows = grid_of(cam, list_px, tile_rows)
    want = ref.expected_lists(order, R, vis, rects, slots, shift, lists_x, row_begin, rows)
    # slot_of_splat is injective over the visible splats, and says "none" exactly for the others
    assert np.unique(slots[vis]).shape[0] == int(vis.sum()) and not (slots[vis] == NONE).any() and (slots[~vis] == NONE).all()
    return ranges, entries, want, (vis, rects, slots, shift, lists_x, row_begin)


def check(mesh, cam, order, R, stats, tile_rows=None):
    """The whole contract of one synchronous draw; returns the model (for the case's own assertions) and the planes."""
    ranges, entries, want, planes = model_of(mesh, cam, order, R, int(stats.list_bin_px), tile_rows)
    why = first_difference(ranges, entries, want, planes[4], planes[5])
    assert np.array_equal(ranges, want.ranges), why
    assert np.array_equal(entries, want.entries), why
    assert int(stats.tile_entries) == want.entries.shape[0] == int(want.runs.sum())
    assert int(stats.visible_splats) == want.walk.shape[0]
    assert int(stats.tiles16) == want.tiles16
    return want, planes


def draw(mesh, cam, order, R, tile_rows=None):
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, R)
    _, stats = mesh.render(tile_rows=tile_rows)
    return stats


# -- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_render_counts_at_the_edges_of_lanes_iterations_and_batches(ctx, R):
    """bin_count_slice: 4 list positions per lane, 1024 per iteration, 256 per batch - the first and the last position of the list
    hold a splat that is certainly drawn, so a slice that loses either end loses an entry."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 5000, seed=11, markers=2)
    n = scene.count
    order = draw_order(scene, cam, permuted=R % 2 == 0, seed=R)
    order = order[order < n - 2][:R].copy()
    order[0] = n - 1                                        # q = R - 1: the last position of the walk
    order[R - 1] = n - 2 if R > 1 else n - 1                # q = 0: the first
    mesh = build_mesh(ctx, scene)
    want, (vis, *_) = check(mesh, cam, order, R, draw(mesh, cam, order, R))
    assert vis[order[0]] and vis[order[R - 1]] and want.walk[0] == order[R - 1] and want.walk[-1] == order[0]
    assert want.walk_q[0] == 0 and want.walk_q[-1] == R - 1 and want.walk.shape[0] > R // 4
    mesh.dispose()


def test_a_grid_at_its_cap_deals_two_batches_per_workgroup(ctx):
    """600 000 list positions: the count's grid stops at 2048 workgroups, so a slice is per = 2 batches and k_bin_emit deals
    (slice, batch) units round-robin.  More than 90 % of the splats are behind the eye or a pixel or two wide."""
    cam = camera.demo_camera("garden", W, H)
    rng = np.random.default_rng(21)
    n = 600_000
    scene = scene_of([placed(cam, 48_000, rng.uniform(0.5, 3.0, 48_000), rng, spread_px=(600.0, 340.0)), behind(cam, n - 48_040, rng),
                      placed(cam, 40, 1500.0, rng, depth=(0.8, 1.5))], 21)
    order = draw_order(scene, cam, permuted=True, seed=21)
    mesh = build_mesh(ctx, scene)
    want, (vis, *_) = check(mesh, cam, order, n, draw(mesh, cam, order, n))
    batches = -(-n // BATCH)
    per = -(-batches // MAX_GRID)
    assert batches > MAX_GRID and per >= 2
    assert 20_000 < vis.sum() < n // 10 and want.entries.shape[0] < 2_000_000
    second = (want.walk_q // BATCH) % per == 1              # survivors in the SECOND batch of their slice, all over the grid
    assert second.sum() > 5_000 and np.unique(want.walk_q[second] // (per * BATCH)).shape[0] > MAX_GRID // 2
    assert (want.runs[second] > 16).any() and (want.runs[~second] > 16).any()
    mesh.dispose()


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 5, 6])
def test_every_list_bin_size(ctx, monkeypatch, shift):
    """rect_to_bins: the four 16-bit fields are shifted in pairs and the bits that cross a field boundary masked; at 512 and 1024 px
    most rects shrink to one bin."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", str(shift))
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 6000, seed=31)
    order = draw_order(scene, cam, permuted=shift % 2 == 1, seed=shift)
    mesh = build_mesh(ctx, scene)                          # the switch is read when the mesh is created
    stats = draw(mesh, cam, order, scene.count)
    assert stats.list_bin_px == 16 << shift
    want, (vis, rects, *_) = check(mesh, cam, order, scene.count, stats)
    x0, y0, x1, y1 = ref.rect_fields(rects[vis])
    low = (1 << shift) - 1
    assert ((y0 & low) != 0).sum() > 100 and ((y1 & low) != 0).sum() > 100     # bits that a plain shift would carry into the x fields
    tiles = ref.bins_of(rects[vis], 0)
    assert ((tiles > 1) & (ref.bins_of(rects[vis], shift) == 1)).sum() > 100    # rects of several tiles inside one list bin
    assert (want.runs > 1).any() or shift == 6
    mesh.dispose()


@pytest.mark.parametrize("w,h,lists", [(512, 512, 256), (544, 512, 272)])
def test_one_pass_and_two_pass_entry_sort_at_their_boundary(ctx, monkeypatch, w, h, lists):
    """256 lists: one radix pass, ranges from the digit totals.  272 lists: two passes, the ranges published with atomics."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = camera.demo_camera("garden", w, h)
    scene = cloud(cam, 5000, seed=41)
    order = draw_order(scene, cam, permuted=lists == 272, seed=41)
    mesh = build_mesh(ctx, scene)
    want, _ = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
    tiles = want.ranges.shape[0]
    assert tiles == lists
    assert (want.ranges[:, 1] > want.ranges[:, 0]).all() and want.entries.shape[0] > 10 * tiles      # every list, also the last, is in use
    mesh.dispose()


@pytest.mark.parametrize("switch", ["GSPLAT_WIDE_ENTRY_KEYS", "GSPLAT_NO_LDS_ATOMIC_RANK"])
def test_context_switches_of_the_entry_sort(monkeypatch, switch):
    """32-bit entry keys (what more than 65536 lists would use), and the entry sort's ballot ranking: a permuted draw order makes
    every list depend on the sort's stability."""
    monkeypatch.setenv(switch, "1")
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")           # 32 x 18 = 576 lists: two passes
    own = Context(0)                                        # the switch is read when the context is created
    try:
        cam = camera.demo_camera("garden", W, H)
        scene = cloud(cam, 20000, seed=51)
        order = draw_order(scene, cam, permuted=True, seed=51)
        mesh = build_mesh(own, scene)
        want, _ = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
        sizes = want.ranges[:, 1].astype(np.int64) - want.ranges[:, 0]
        assert want.ranges.shape[0] == 576 and (sizes > 64).sum() > 288  # lists longer than a wave: equal digits meet in one wave
    finally:
        own.close()                                         # (with its meshes, also when the comparison fails)


def test_the_walk_without_the_lds_block_bitmap(ctx, monkeypatch):
    """GSPLAT_NO_COARSE_VIS=1: the count tests the flag byte of a list position's storage block instead of the bitmap in LDS (what
    a mesh of more than 65536 blocks does).  Storage in upload order, three whole blocks of it behind the eye: the positions of a
    dead block must be dropped by the flag, the vertex stage left no word to gather for them."""
    monkeypatch.setenv("GSPLAT_NO_COARSE_VIS", "1")
    cam = camera.demo_camera("garden", W, H)
    rng = np.random.default_rng(61)
    front = helpers.small_scene(4000, 0, 61)
    scene = scene_of([(front.centers[:512], front.cov[:512]), behind(cam, 768, rng), (front.centers[512:], front.cov[512:]),
                      placed(cam, 6, 1500.0, rng, depth=(0.8, 1.5))], 61)
    order = draw_order(scene, cam, permuted=False)
    mesh = build_mesh(ctx, scene, keep_order=True)
    want, (vis, *_) = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
    assert not vis[512:1280].any() and vis[:512].sum() > 100 and vis[1280:].sum() > 1000
    assert np.isin(np.arange(512, 1280), order).all()       # the list does name the splats of the dead blocks
    mesh.dispose()


def test_runs_of_every_length_in_one_batch(ctx, monkeypatch):
    """EMIT_OWN = 16: a lane writes the first 16 entries of its splat, the wave shares what is left.  Splats of 1, 2-16, 17-64 and
    more than 500 list bins, interleaved in depth, meet in every batch of 256."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = camera.demo_camera("garden", W, H)
    rng = np.random.default_rng(71)
    scene = scene_of([placed(cam, 1400, 3.0, rng), placed(cam, 1000, 30.0, rng), placed(cam, 1000, rng.uniform(65.0, 85.0, 1000), rng),
                      placed(cam, 150, 1500.0, rng, spread_px=(100.0, 60.0))], 71)
    order = draw_order(scene, cam, permuted=False)          # true depth order: all four kinds lie between 2 and 6 in front of the eye
    mesh = build_mesh(ctx, scene)
    want, _ = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
    batch = want.walk_q // BATCH
    kinds = [want.runs == 1, (want.runs >= 2) & (want.runs <= 16), (want.runs >= 17) & (want.runs <= 64), want.runs > 500]
    per_batch = np.stack([np.bincount(batch[k], minlength=int(batch.max()) + 1) for k in kinds])
    long_runs, short_runs = per_batch[2] + per_batch[3], per_batch[0] + per_batch[1]
    assert ((long_runs >= 50) & (short_runs >= 50) & (per_batch >= 4).all(axis=0)).any(), per_batch.T.tolist()
    mesh.dispose()


@pytest.mark.parametrize("keep_order", [False, True])
def test_the_caller_numbering_is_translated_to_storage_order(ctx, keep_order):
    """`perm`: the render list names splats as the caller uploaded them, the storage is in Morton order unless keep_order."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 4000, seed=81)
    order = draw_order(scene, cam, permuted=keep_order, seed=81)
    mesh = build_mesh(ctx, scene, keep_order=keep_order)
    want, (vis, _, slots, *_) = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
    rising = (np.diff(slots[vis].astype(np.int64)) > 0).all()
    assert rising == keep_order and vis.sum() > 1000       # slots follow the upload order only when the storage does
    mesh.dispose()


def test_duplicates_stale_indexes_and_a_short_render_count(ctx):
    """Every occurrence of an index emits; indexes >= the splat count draw nothing (and fault nothing); positions past render_count
    are never read."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 5000, seed=91, markers=4)
    n = scene.count
    order = draw_order(scene, cam, permuted=True, seed=91)
    order[::5] = n - 1                                      # a marker, a thousand times
    order[3::7] = 0xFFFFFFF0
    order[6::49] = n                                        # the first index that is none
    R = n - 1000
    order[R:] = n - 2                                       # must not show: another marker
    mesh = build_mesh(ctx, scene)
    want, (vis, *_) = check(mesh, cam, order, R, draw(mesh, cam, order, R))
    assert vis[n - 1] and vis[n - 2] and (want.walk == n - 1).sum() == (order[:R] == n - 1).sum() > 500
    assert not (want.walk == n - 2).any() and (order[:R] >= n).sum() > 500
    mesh.dispose()


@pytest.mark.parametrize("seen", ["nothing", "first position", "last position"])
def test_an_empty_frame_and_a_single_splat(ctx, seen):
    """Nothing visible: every range reads (~0, 0) and there is no entry.  One visible splat at either end of the list: its bins,
    nothing else."""
    cam = camera.demo_camera("garden", W, H)
    rng = np.random.default_rng(101)
    scene = scene_of([behind(cam, 2999, rng), placed(cam, 1, 60.0, rng) if seen != "nothing" else behind(cam, 1, rng)], 101)
    n = scene.count
    order = np.arange(n, dtype=np.uint32)                   # the one in front is the last index
    if seen == "first position":
        order = order[::-1].copy()
    mesh = build_mesh(ctx, scene)
    stats = draw(mesh, cam, order, n)
    want, (vis, *_) = check(mesh, cam, order, n, stats)
    ranges, entries, _ = mesh.bin_lists()
    if seen == "nothing":
        assert not vis.any() and entries.shape[0] == 0 and (ranges == ref.UNTOUCHED).all() and ranges.shape[0] == 8 * 5
    else:
        assert vis.sum() == 1 and vis[n - 1] and want.walk_q.tolist() == [0 if seen == "last position" else n - 1]
        assert entries.shape[0] == want.runs[0] >= 1 and (ranges[:, 1] > ranges[:, 0]).sum() == want.runs[0]
    mesh.dispose()


@pytest.mark.parametrize("rows", [(0, 11), (11, 36), (3, 4)])
def test_strips_number_their_lists_from_their_own_first_row(ctx, rows):
    """list_row_begin: at 128-px lists tile row 11 lies inside list-bin row 1.  The lists of a strip are the model's, built from the
    rects the vertex stage clipped to that strip."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 6000, seed=111)
    order = draw_order(scene, cam, permuted=rows[0] == 11, seed=111)
    mesh = build_mesh(ctx, scene)
    stats = draw(mesh, cam, order, scene.count, tile_rows=rows)
    assert stats.list_bin_px == 128
    want, (vis, rects, _, shift, lists_x, row_begin) = check(mesh, cam, order, scene.count, stats, tile_rows=rows)
    assert (row_begin, want.ranges.shape[0]) == {(0, 11): (0, 8 * 2), (11, 36): (1, 8 * 4), (3, 4): (0, 8 * 1)}[rows]
    _, y0, _, y1 = ref.rect_fields(rects[vis])
    assert y0.min() == rows[0] and y1.max() == min(rows[1], 36) - 1 and want.entries.shape[0] > 500
    mesh.dispose()


@pytest.mark.parametrize("cull", ["frustum", "visibility"])
def test_a_list_whose_length_only_the_device_knows(ctx, cull):
    """R_dev: after a culled sort the result's length lives on the device; the binner walks min(kept, render_count) positions of
    a grid sized for render_count."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 8000, seed=121)
    n = scene.count
    mvp = cam.sort_mvp()
    w = create_sort_worker(ctx, n)
    w.post_message({"centers": util.integer_centers(scene.centers), "range": {"from": 0, "to": n - 1, "count": n}})
    mesh = build_mesh(ctx, scene)
    mesh.set_camera(cam)
    mesh.use_sorter_result(w, n)                            # binds: the next sort hands over storage positions
    if cull == "frustum":
        w.set_frustum_cull(True)
    else:
        w.set_visibility_cull(True)
        mesh.project()
    w.sort_on_device(mvp, n)
    _, stats = mesh.render()
    kept = int(w.last_stats()[0].result_count)
    order = w.debug_read(2, kept)                           # the kept list in the caller's numbering
    want, (vis, *_) = check(mesh, cam, order, kept, stats)
    assert 1000 < kept < n - 500 and -(-kept // BATCH) < -(-n // BATCH)
    assert want.walk.shape[0] == vis.sum() and (cull == "frustum" or kept == vis.sum())
    if cull == "visibility":                                # what = 8 refuses while a vertex stage for the NEXT frame is pending
        mesh.project()
        with pytest.raises(L.GsError):
            mesh.bin_lists()
    w.terminate()
    mesh.dispose()


def test_lists_of_a_permuted_order_over_many_count_slices(ctx):
    """20000 splats in a permuted draw order: more than 64 batches of 256 list positions, so k_bin_emit's scan of the count
    workgroups' sums and its round-robin deal of batches run over many slices."""
    cam = camera.demo_camera("garden", W, H)
    scene = cloud(cam, 20000, seed=131)
    order = draw_order(scene, cam, permuted=True, seed=131)
    mesh = build_mesh(ctx, scene)
    want, _ = check(mesh, cam, order, scene.count, draw(mesh, cam, order, scene.count))
    assert -(-scene.count // BATCH) > 64 and want.entries.shape[0] > 20000
    mesh.dispose()


def crowded(cam, seed):
    """A few thousand splats of 20-90 px: tens of thousands of entries at 32-px lists."""
    rng = np.random.default_rng(seed)
    return scene_of([placed(cam, 3000, rng.uniform(20.0, 90.0, 3000), rng), placed(cam, 6, 1500.0, rng, depth=(0.8, 1.5))], seed)


def test_a_draw_that_overflows_is_redone_completely(ctx, monkeypatch):
    """Entry capacity 4096 and a synchronous draw: the buffers grow and the draw is repeated; the lists are complete."""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = camera.demo_camera("garden", W, H)
    scene = crowded(cam, 141)
    order = draw_order(scene, cam, permuted=False)
    mesh = build_mesh(ctx, scene)
    mesh.debug_set_entry_capacity(4096)
    stats = draw(mesh, cam, order, scene.count)
    want, _ = check(mesh, cam, order, scene.count, stats)
    assert stats.overflowed == 1 and want.entries.shape[0] > 10 * 4096 and stats.entry_capacity >= want.entries.shape[0]
    mesh.dispose()


def test_a_truncated_draw_keeps_a_prefix_of_the_walk(ctx, monkeypatch):
    """An asynchronous draw cannot redo itself: what does not fit is dropped.  It keeps the first `capacity` entries of the walk:
    every list is a prefix of the model's, every splat is wholly there or wholly missing except at most one at the cut, and every
    splat that is there is nearer than every missing one.  (None of this depends on the order of the bins inside a splat's run.)"""
    monkeypatch.setenv("GSPLAT_LIST_SHIFT", "1")
    cam = camera.demo_camera("garden", W, H)
    scene = crowded(cam, 151)
    order = draw_order(scene, cam, permuted=True, seed=151)
    cap = 4096 + 37
    mesh = build_mesh(ctx, scene)
    mesh.debug_set_entry_capacity(cap)
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, scene.count)
    mesh.render(to_host=False, want_stats=False)            # nobody looks: no regrow, no redraw
    ctx.synchronize()
    ranges, entries, want, _ = model_of(mesh, cam, order, scene.count, 32)       # (last_stats() would heal the buffers)
    assert want.entries.shape[0] > 10 * cap and entries.shape[0] == cap
    got_len = np.where(ranges[:, 1] > ranges[:, 0], ranges[:, 1].astype(np.int64) - ranges[:, 0], 0)
    want_len = want.ranges[:, 1].astype(np.int64) - np.minimum(want.ranges[:, 0], want.ranges[:, 1])
    assert got_len.sum() == cap and (got_len <= want_len).all()
    touched = got_len > 0
    assert np.array_equal(ranges[touched, 0], np.cumsum(got_len)[touched] - got_len[touched])       # the lists tile [0, capacity)
    kept = np.zeros(want.entries.shape[0], dtype=bool)     # the model's entries that a prefix of every list keeps
    for i in np.nonzero(touched)[0]:
        b, wb = int(ranges[i, 0]), int(want.ranges[i, 0])
        assert np.array_equal(entries[b:b + got_len[i]], want.entries[wb:wb + got_len[i]]), f"list {i} is not a prefix of the model's"
        kept[wb:wb + got_len[i]] = True
    present = np.bincount(want.entry_walk[kept], minlength=want.walk.shape[0])
    whole, partial, absent = (present == want.runs) & (want.runs > 0), (present > 0) & (present < want.runs), (present == 0) & (want.runs > 0)
    assert partial.sum() <= 1 and whole.sum() > 20 and absent.sum() > 20
    first_absent = int(np.nonzero(absent)[0].min())
    assert np.nonzero(whole)[0].max() < first_absent and (not partial.any() or np.nonzero(partial)[0][0] < first_absent)
    assert not partial.any() or np.nonzero(whole)[0].max() < np.nonzero(partial)[0][0]
    mesh.dispose()
