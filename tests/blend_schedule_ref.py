"""Host model of the blend schedule (gaussiansplats3d_amd/csrc/tile_bin.hip, blend_schedule_job): exact Python integers, none of
the kernel's uint32 arithmetic.  Where the kernel is right the two agree to the bit; where a uint32 sum or product would wrap,
this model keeps the true value and the GPU test that holds the kernel to it fails.

Read next to the kernel:
  cost_of(i)        -> shifted_costs: bin i = (bx, by) reads the previous draw's .y of bin (bx - sx, by - sy), 0 off the frame
  total_walked      -> Schedule.total: the sum of those costs
  shift             -> Schedule.shift: the smallest s with (total // B) >> s <= 48
  255 - min(c >> s, 255) -> Schedule.keys, and their counting sort's buckets -> Schedule.buckets
  mean_halves, deep_trigger, deep_thr -> Schedule.mean, .trigger, .thr
  the head of the order, its members, s_trigger, mirror[4], mirror[5] -> head_outcome()
"""
from dataclasses import dataclass

import numpy as np

DEEP_MAX_BINS = 512        # GS_DEEP_MAX_BINS: the deep pass's members come from the first 512 bins of the order
KEY_MEAN = 48              # the mean bin's 8-bit cost lands at or below this


def shifted_costs(stats_y, bins_x, blend_bins, sx, sy):
    """Per bin of this draw: the cost (.y of the previous draw's per-bin statistics) of the bin its content came from."""
    y = [int(v) for v in np.asarray(stats_y).reshape(-1)[:blend_bins]]
    assert len(y) == blend_bins and blend_bins % bins_x == 0
    rows = blend_bins // bins_x
    out = []
    for i in range(blend_bins):
        by, bx = divmod(i, bins_x)
        fx, fy = bx - sx, by - sy
        out.append(y[fy * bins_x + fx] if 0 <= fx < bins_x and 0 <= fy < rows else 0)
    return out


@dataclass
class Schedule:
    costs: list
    total: int
    shift: int
    keys: list
    buckets: list
    mean: int
    trigger: int
    thr: int


def schedule(stats_y, bins_x, blend_bins, sx, sy, deep_min, deep_factor):
    costs = shifted_costs(stats_y, bins_x, blend_bins, sx, sy)
    total = sum(costs)
    shift = 0
    while (total // blend_bins) >> shift > KEY_MEAN:
        shift += 1
    keys = [255 - min(c >> shift, 255) for c in costs]
    buckets = [0] * 256
    for k in keys:
        buckets[k] += 1
    mean = total // max(blend_bins, 1)
    trigger = max(2 * deep_min, deep_factor * mean)
    thr = max(2 * deep_min, mean - mean // 4)
    return Schedule(costs, total, shift, keys, buckets, mean, trigger, thr)


def head_outcome(sch, order):
    """What the kernel must decide from the head of ITS order (the order inside a bucket is free, so the head is taken from
    the kernel): {members (set), candidates (mirror[4]), share (mirror[5])}."""
    head = [int(i) for i in order[:min(len(order), DEEP_MAX_BINS)]]
    members = {i for i in head if sch.costs[i] >= sch.thr}
    fired = any(sch.costs[i] >= sch.trigger for i in head)
    share = (sum(sch.costs[i] >> 4 for i in members) << 14) // max(sch.total, 1)
    return {"members": members, "candidates": len(members) if fired else 0, "share": share}


def check_order(sch, order):
    """The order is a permutation of the bins whose keys never decrease, with the model's bucket counts.  Returns a list of
    what is wrong (empty when nothing is)."""
    order = [int(i) for i in order]
    n = len(sch.costs)
    bad = []
    if sorted(order) != list(range(n)):
        bad.append("the order is not a permutation of the bins")
        return bad
    keys = [sch.keys[i] for i in order]
    drops = [p for p in range(1, n) if keys[p] < keys[p - 1]]
    if drops:
        bad.append(f"keys decrease along the order at positions {drops[:8]}")
    counts = [0] * 256
    for k in keys:
        counts[k] += 1
    if counts != sch.buckets:
        bad.append("bucket counts differ")
    return bad
