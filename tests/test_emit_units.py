"""k_bin_emit's live units (csrc/draw_plan.hpp: live_batches, live_unit_word, live_unit_find) through the library's pure-host debug
entry gs_debug_live_units: no GPU.  The entry packs one word per slice the way the kernel's prologue does and looks every unit up
with the function the kernel searches its LDS with.  What must hold, against brute force over the slices' counts: every batch that
holds a splat is dealt exactly once, in walk order, with the number of splats it holds, and no empty batch is dealt."""
import ctypes as C

import numpy as np
import pytest

import gaussiansplats3d_amd as g

BATCH, SLICES = 256, 2048             # GS_EMIT_BATCH, and BIN_MAX_BLOCKS of tile_bin.hip


def live_units(cnt, room=None):
    fn = g.load().gs_debug_live_units
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    room = int(-(-cnt.astype(np.int64) // BATCH).sum()) + 3 if room is None else room
    out = np.full((room, 3), 0xDEADBEEF, dtype=np.uint32)
    total = fn(cnt.ctypes.data, cnt.shape[0], out.ctypes.data, room)
    return total, out


def brute_force(cnt):
    return [(b, j, min(BATCH, int(c) - BATCH * j)) for b, c in enumerate(cnt) for j in range(-(-int(c) // BATCH))]


def check(cnt):
    want = brute_force(cnt)
    total, out = live_units(cnt)
    assert total == len(want)
    got = [tuple(int(v) for v in row) for row in out[:total]]
    assert got == want                                      # walk order: slice by slice, batch by batch
    assert len(set(got)) == len(got)                        # ... so every live (slice, batch) exactly once, and no dead one
    assert (out[total:] == 0xDEADBEEF).all()                # nothing is written past the draw's units
    # the round-robin deal l = wg, wg + wgs, ... of any grid covers 0 .. total - 1 once
    for wgs in (1, 7, SLICES):
        dealt = np.concatenate([np.arange(wg, total, wgs) for wg in range(wgs)]) if total else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(dealt), np.arange(total))
    return want


def test_null_arguments_and_no_slices_are_refused():
    fn = g.load().gs_debug_live_units
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    one = np.ones(1, dtype=np.uint32)
    assert fn(None, 1, None, 0) == -1
    assert fn(one.ctypes.data, 0, None, 0) == -1
    assert fn(one.ctypes.data, 1, None, 4) == -1
    assert fn(one.ctypes.data, 1, None, 0) == 1             # only the count


@pytest.mark.parametrize("slices", [1, 3, 100, SLICES])
def test_nothing_visible_deals_nothing(slices):
    assert check(np.zeros(slices, dtype=np.uint32)) == []


@pytest.mark.parametrize("per", [1, 12, 31])
@pytest.mark.parametrize("slices", [1, 5, SLICES])
def test_every_slice_full(per, slices):
    want = check(np.full(slices, per * BATCH, dtype=np.uint32))
    assert len(want) == per * slices and all(c == BATCH for _, _, c in want)


@pytest.mark.parametrize("per", [2, 31])
def test_counts_at_the_edges_of_a_batch_mixed(per):
    """0 / 1 / 256 / 257 / 512 in every order of neighbours (a seeded shuffle of many of each), and in a fixed run that puts
    each next to each."""
    values = np.array([0, 1, 256, 257, 512], dtype=np.uint32)
    assert per * BATCH >= 512
    pairs = np.array([v for a in values for b in values for v in (a, b)], dtype=np.uint32)
    check(pairs)
    rng = np.random.default_rng(13)
    check(rng.choice(values, size=SLICES))
    check(np.concatenate([np.zeros(700, np.uint32), rng.choice(values, size=SLICES - 1400), np.zeros(700, np.uint32)]))


@pytest.mark.parametrize("per", [1, 31])
@pytest.mark.parametrize("where", [0, SLICES - 1])
@pytest.mark.parametrize("count", [1, 255, 256, "full", "full - 1"])
def test_a_single_live_slice_at_either_end(per, where, count):
    count = {"full": per * BATCH, "full - 1": per * BATCH - 1}.get(count, count)
    assert count <= per * BATCH
    cnt = np.zeros(SLICES, dtype=np.uint32)
    cnt[where] = count
    want = check(cnt)
    assert {b for b, _, _ in want} == {where} and sum(c for _, _, c in want) == count


@pytest.mark.parametrize("per", [1, 31])
def test_random_counts(per):
    rng = np.random.default_rng(per)
    for slices in (2, 17, SLICES):
        cnt = rng.integers(0, per * BATCH + 1, size=slices).astype(np.uint32)
        cnt[rng.random(slices) < 0.4] = 0                   # runs of empty slices: words that share a first unit
        want = check(cnt)
        assert sum(c for _, _, c in want) == int(cnt.sum())


def test_a_quarter_full_draw_like_the_flagship():
    """12 batches per slice of which about three hold something: the shape whose empty batches the deal used to hand out."""
    rng = np.random.default_rng(3)
    cnt = np.minimum(rng.poisson(765, size=SLICES), 12 * BATCH).astype(np.uint32)
    cnt[1888:] = 0
    want = check(cnt)
    assert 5000 < len(want) < 8000


def test_the_room_bounds_what_is_written():
    cnt = np.full(8, 3 * BATCH, dtype=np.uint32)
    total, out = live_units(cnt, room=5)
    assert total == 24
    assert [tuple(int(v) for v in r) for r in out] == brute_force(cnt)[:5]
