"""CPU tier: the host model of the binner's entry lists (bin_lists_ref.py) against a brute-force triple loop - per list bin, per
list position from the end, per splat: does its rect touch the bin? - on hand-written inputs of a few dozen splats."""
import numpy as np
import pytest

import bin_lists_ref as ref


def rect(x0, y0, x1, y1):
    return [x0 | (y0 << 16), x1 | (y1 << 16)]


def brute_force(order, R, visible, rects, slots, shift, lists_x, row_begin, rows):
    lists = []
    for ly in range(row_begin, row_begin + rows):
        for lx in range(lists_x):
            mine = []
            for p in range(R - 1, -1, -1):
                i = int(order[p])
                if i >= len(visible) or not visible[i]:
                    continue
                x0, y0 = (rects[i][0] & 0xFFFF) >> shift, (rects[i][0] >> 16) >> shift
                x1, y1 = (rects[i][1] & 0xFFFF) >> shift, (rects[i][1] >> 16) >> shift
                if x0 <= lx <= x1 and y0 <= ly <= y1:
                    mine.append(int(slots[i]))
            lists.append(mine)
    ranges, entries = [], []
    for mine in lists:
        ranges.append([len(entries), len(entries) + len(mine)] if mine else list(ref.UNTOUCHED))
        entries += mine
    return np.array(ranges, dtype=np.uint32).reshape(-1, 2), np.array(entries, dtype=np.uint32)


def scene(n=40, tiles_x=24, row0=0, row1=20, seed=1):
    """n splats with rects inside tile columns [0, tiles_x) and tile rows [row0, row1): a mix of single tiles, rects across
    bin boundaries and a few that cover most of the grid; every fifth splat invisible; slots scattered and unique."""
    rng = np.random.default_rng(seed)
    rects = []
    for i in range(n):
        w, h = ((1, 1), (2, 3), (5, 2), (tiles_x - 2, row1 - row0 - 1))[i % 4]
        h = min(max(h, 1), row1 - row0)
        x0, y0 = int(rng.integers(0, tiles_x - w + 1)), int(rng.integers(row0, row1 - h + 1))
        rects.append(rect(x0, y0, x0 + w - 1, y0 + h - 1))
    visible = np.array([i % 5 != 3 for i in range(n)])
    slots = np.where(visible, rng.permutation(n) * 3 + 7, 0xFFFFFFFF).astype(np.uint32)
    rects = np.array(rects, dtype=np.uint32)
    rects[~visible] = (0xFFFF, 0)                          # what the rect plane holds for a culled splat
    return visible, rects, slots


def check(order, R, visible, rects, slots, shift, lists_x, row_begin, rows):
    got = ref.expected_lists(order, R, visible, rects, slots, shift, lists_x, row_begin, rows)
    ranges, entries = brute_force(order, R, visible, rects, slots, shift, lists_x, row_begin, rows)
    np.testing.assert_array_equal(got.ranges, ranges)
    np.testing.assert_array_equal(got.entries, entries)
    assert got.runs.sum() == len(entries) and got.entries.dtype == np.uint32 and got.ranges.dtype == np.uint32
    np.testing.assert_array_equal(slots[got.walk][got.entry_walk], got.entries)
    return got


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5])
def test_model_equals_the_triple_loop_at_every_list_bin_size(shift):
    visible, rects, slots = scene()
    n = len(visible)
    order = np.random.default_rng(2).permutation(n).astype(np.uint32)
    lists_x, rows = ((24 - 1) >> shift) + 1, ((20 - 1) >> shift) + 1
    got = check(order, n, visible, rects, slots, shift, lists_x, 0, rows)
    assert len(got.walk) == visible.sum() and got.tiles16 == ref.bins_of(rects[visible], 0).sum()
    if shift == 5:                                         # one list: the walk itself
        np.testing.assert_array_equal(got.entries, slots[order[::-1]][visible[order[::-1]]])


def test_duplicates_out_of_range_indexes_and_a_short_render_count():
    visible, rects, slots = scene(seed=3)
    n = len(visible)
    order = np.arange(n, dtype=np.uint32)[::-1].copy()
    order[5] = order[20]                                   # a duplicate: both occurrences emit
    order[9] = n                                           # the first index past the splats
    order[11] = 0xFFFFFFF0
    assert visible[order[5]] and visible[order[10]]
    R = 30                                                 # < n: positions 30.. are never read
    order[R:] = 0xFFFFFFFF
    got = check(order, R, visible, rects, slots, 1, 12, 0, 10)
    assert (got.walk == order[5]).sum() == 2
    assert len(got.walk) == sum(1 for p in range(R) if order[p] < n and visible[order[p]])


def test_a_rect_across_a_bin_boundary_lands_in_every_bin_it_touches_once():
    visible = np.array([True, True])
    rects = np.array([rect(3, 1, 4, 2), rect(4, 2, 4, 2)], dtype=np.uint32)     # 64-px bins: tiles 3|4 and 1|2 are boundaries
    slots = np.array([70, 50], dtype=np.uint32)
    got = check(np.array([0, 1], np.uint32), 2, visible, rects, slots, 2, 2, 0, 1)
    np.testing.assert_array_equal(got.ranges, [[0, 1], [1, 3]])
    np.testing.assert_array_equal(got.entries, [70, 50, 70])                     # list 1: splat 1 is drawn last = nearest = first
    got = check(np.array([0, 1], np.uint32), 2, visible, rects, slots, 0, 5, 1, 2)
    E = list(ref.UNTOUCHED)
    np.testing.assert_array_equal(got.ranges, [E, E, E, [0, 1], [1, 2], E, E, E, [2, 3], [3, 5]])
    np.testing.assert_array_equal(got.entries, [70, 70, 70, 50, 70])


@pytest.mark.parametrize("row0,row1,shift", [(8, 20, 2), (3, 4, 3), (11, 36, 3)])
def test_a_strip_numbers_its_lists_from_its_own_first_row(row0, row1, shift):
    """list_row_begin > 0, also for a strip that starts inside a list-bin row (tile row 11 of 128-px lists = list row 1)."""
    visible, rects, slots = scene(n=36, tiles_x=30, row0=row0, row1=row1, seed=row0)
    n = len(visible)
    order = np.random.default_rng(5).permutation(n).astype(np.uint32)
    row_begin, row_end = row0 >> shift, ((row1 - 1) >> shift) + 1
    got = check(order, n, visible, rects, slots, shift, ((30 - 1) >> shift) + 1, row_begin, row_end - row_begin)
    assert got.ranges.shape[0] == (((30 - 1) >> shift) + 1) * (row_end - row_begin) and len(got.entries) > 0


def test_nothing_visible_and_an_empty_render_list():
    visible, rects, slots = scene()
    n = len(visible)
    order = np.arange(n, dtype=np.uint32)
    for got in (ref.expected_lists(order, n, np.zeros(n, bool), rects, slots, 1, 12, 0, 10),
                ref.expected_lists(order, 0, visible, rects, slots, 1, 12, 0, 10)):
        assert got.entries.shape == (0,) and got.tiles16 == 0 and len(got.walk) == 0
        assert (got.ranges == ref.UNTOUCHED).all() and got.ranges.shape == (120, 2)


def test_a_rect_outside_the_strip_is_an_input_error():
    with pytest.raises(ValueError):
        ref.expected_lists([0], 1, [True], [rect(0, 0, 0, 0)], [0], 0, 4, 1, 2)
    with pytest.raises(ValueError):
        ref.expected_lists([0], 1, [True], [rect(3, 1, 4, 1)], [0], 0, 4, 1, 2)
