"""CPU tier: the host model of the blend schedule (blend_schedule_ref.py) on small grids computed by hand."""
import numpy as np

import blend_schedule_ref as ref

# 4 x 3 bins, costs 0..110 in row-major order
GRID = [0, 10, 20, 30,
        40, 50, 60, 70,
        80, 90, 100, 110]


def costs(sx, sy, stats=GRID, bx=4, B=12):
    return ref.shifted_costs(np.array(stats), bx, B, sx, sy)


def test_no_shift_reads_every_bin_itself():
    assert costs(0, 0) == GRID


def test_positive_shift_reads_left_and_up_and_zeroes_the_edges_it_uncovers():
    # bin (x, y) reads (x - 1, y - 1): column 0 and row 0 come from outside the frame
    assert costs(1, 1) == [0, 0, 0, 0,
                           0, 0, 10, 20,
                           0, 40, 50, 60]


def test_negative_shift_reads_right_and_down():
    # bin (x, y) reads (x + 2, y + 1): the last two columns and the last row fall off the right / bottom edge
    assert costs(-2, -1) == [60, 70, 0, 0,
                             100, 110, 0, 0,
                             0, 0, 0, 0]


def test_shift_on_one_axis_only():
    assert costs(-1, 0) == [10, 20, 30, 0, 50, 60, 70, 0, 90, 100, 110, 0]
    assert costs(0, 2) == [0] * 8 + [0, 10, 20, 30]
    assert costs(0, -2) == [80, 90, 100, 110] + [0] * 8


def test_shift_larger_than_the_frame_reads_nothing():
    for sx, sy in ((4, 0), (-4, 0), (0, 3), (0, -3), (100, -100)):
        assert costs(sx, sy) == [0] * 12


def test_a_row_never_wraps_into_its_neighbour():
    # row-major index arithmetic alone would read bin 3 (end of row 0) for bin 4 (start of row 1) at sx = 1
    assert costs(1, 0)[4] == 0 and costs(-1, 0)[3] == 0


def test_scale_shift_keys_buckets_and_thresholds():
    # total 660, B 12: mean 55 > 48 -> s = 1 (55 >> 1 = 27)
    sch = ref.schedule(np.array(GRID), 4, 12, 0, 0, deep_min=20, deep_factor=2)
    assert sch.total == 660 and sch.shift == 1 and sch.mean == 55
    assert sch.keys == [255 - c // 2 for c in GRID]
    assert sum(sch.buckets) == 12 and sch.buckets[255] == 1 and sch.buckets[200] == 1
    assert sch.trigger == max(40, 110) == 110
    assert sch.thr == max(40, 55 - 13) == 42


def test_shift_is_the_smallest_that_brings_the_mean_to_48():
    for mean, want in ((0, 0), (48, 0), (49, 1), (97, 1), (98, 2), (48 << 5, 5), ((48 << 5) + 32, 6)):
        sch = ref.schedule(np.full(4, mean), 2, 4, 0, 0, 0, 3)
        assert sch.mean == mean and sch.shift == want, (mean, sch.shift)


def test_keys_saturate_at_zero():
    sch = ref.schedule(np.array([0, 0, 0, 10_000]), 2, 4, 0, 0, 0, 3)    # mean 2500 -> s = 6; 10000 >> 6 = 156
    assert sch.shift == 6 and sch.keys == [255, 255, 255, 99]
    sch = ref.schedule(np.array([0] * 15 + [100_000]), 4, 16, 0, 0, 0, 3)  # mean 6250 -> s = 8; 100000 >> 8 = 390 -> 255
    assert sch.keys[15] == 0


def test_ties_share_a_bucket_and_either_order_passes():
    sch = ref.schedule(np.array([5, 7, 7, 5]), 2, 4, 0, 0, 0, 3)
    assert sch.keys[1] == sch.keys[2] and sch.buckets[sch.keys[1]] == 2
    assert ref.check_order(sch, [1, 2, 0, 3]) == [] and ref.check_order(sch, [2, 1, 3, 0]) == []
    assert ref.check_order(sch, [0, 1, 2, 3]) != []          # a cheap bin ahead of a costly one
    assert ref.check_order(sch, [1, 1, 0, 3]) != []          # not a permutation


def test_head_members_trigger_and_share():
    sch = ref.schedule(np.array(GRID), 4, 12, 0, 0, deep_min=20, deep_factor=2)   # thr 42, trigger 110
    order = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    out = ref.head_outcome(sch, order)
    assert out["members"] == {5, 6, 7, 8, 9, 10, 11}                           # costs 50 .. 110 >= 42
    assert out["candidates"] == 7                                              # bin 11 reaches the trigger
    assert out["share"] == ((3 + 3 + 4 + 5 + 5 + 6 + 6) << 14) // 660         # sum of c >> 4
    sch2 = ref.schedule(np.array(GRID), 4, 12, 0, 0, deep_min=20, deep_factor=3)  # trigger 165: nobody reaches it
    assert ref.head_outcome(sch2, order)["candidates"] == 0
    assert ref.head_outcome(sch2, order)["members"] == out["members"]          # members do not depend on the trigger


def test_only_the_head_of_the_order_can_hold_members():
    B = 600
    sch = ref.schedule(np.full(B, 9000), 20, B, 0, 0, deep_min=4096, deep_factor=3)
    assert sch.thr == 8192
    order = list(range(B))
    assert ref.head_outcome(sch, order)["members"] == set(range(ref.DEEP_MAX_BINS))


def test_total_above_2_32_is_kept_exactly():
    B = 8192
    stats = np.full(B, 1 << 20, dtype=np.uint64)       # 2^33 in all: a uint32 sum would wrap to 0
    sch = ref.schedule(stats, 128, B, 0, 0, deep_min=4096, deep_factor=3)
    assert sch.total == 1 << 33 and sch.mean == 1 << 20
    assert sch.shift == 15                             # 2^20 >> 15 = 32 <= 48, >> 14 = 64 > 48
    assert sch.trigger == 3 << 20 and sch.thr == (1 << 20) - (1 << 18)
    out = ref.head_outcome(sch, list(range(B)))
    assert len(out["members"]) == 512
    assert out["share"] == ((512 * (1 << 16)) << 14) // (1 << 33)          # 512 of 8192 bins = 1/16 of 1024 = 64
    assert out["share"] == 64
