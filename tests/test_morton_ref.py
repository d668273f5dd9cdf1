"""CPU tier: the numpy model of a Morton run's storage order (morton_ref.py) does what its docstring says before the GPU tests rely
on it - the bounds' treatment of NaN and infinities, 30-bit codes against a scalar re-computation, the tie order."""
import numpy as np

import helpers
import morton_ref


def _scalar_key(c, mn, mx):
    """one splat, bit by bit, in float32 scalars"""
    key = 0
    for k in range(3):
        inv = np.float32(1.0) / np.float32(mx[k] - mn[k]) if mx[k] > mn[k] else np.float32(0.0)
        with np.errstate(all="ignore"):
            t = np.float32(np.float32(np.float32(c[k] - mn[k]) * inv) * np.float32(1023.0))
        q = 0 if np.isnan(t) or t < 0 else (1023 if t > 1023 else int(t))
        for bit in range(10):
            key |= ((q >> bit) & 1) << (3 * bit + k)
    return key


def test_keys_equal_a_scalar_recomputation():
    c = helpers.small_scene(500, 0, 3).centers.copy()
    c[7, 0], c[9, 2], c[11, 1] = np.nan, -np.inf, c[:, 1].max()
    mn, mx = morton_ref.bounds(c)
    assert mn[2] == -np.inf and np.isfinite(mn[:2]).all() and np.isfinite(mx).all()     # NaN moved nothing, the infinity did
    keys = morton_ref.keys(c)
    assert keys.dtype == np.uint32 and int(keys.max()) < 1 << 30
    assert [int(k) for k in keys] == [_scalar_key(c[i], mn, mx) for i in range(len(c))]
    assert not (keys & np.uint32(0x24924924)).any()        # z: an infinite extent gives every splat code 0 on that axis
    assert int(keys[7]) & 0x09249249 == 0                  # a NaN coordinate is code 0


def test_an_axis_of_extent_zero_and_no_finite_centre():
    c = helpers.small_scene(100, 0, 4).centers.copy()
    c[:, 1] = c[0, 1]
    assert not (morton_ref.keys(c) & np.uint32(0x12492492)).any()
    nothing = np.full((5, 3), np.nan, np.float32)
    mn, mx = morton_ref.bounds(nothing)
    assert (mn == np.inf).all() and (mx == -np.inf).all() and not morton_ref.keys(nothing).any()


def test_equal_keys_keep_the_original_index_order():
    c = helpers.small_scene(300, 0, 5).centers
    twice = np.concatenate([c, c])
    order, pos = morton_ref.order(twice), morton_ref.positions(twice, 1000)
    assert sorted(order.tolist()) == list(range(600)) and sorted(pos.tolist()) == list(range(1000, 1600))
    assert (pos[:300] < pos[300:]).all()
    keys = morton_ref.keys(twice)[order]
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    same = np.flatnonzero(np.diff(keys.astype(np.int64)) == 0)
    assert same.size >= 300 and (order[same] < order[same + 1]).all()
