"""CPU tier: whether a static integer sorter's centres fit 16-bit offset planes (csrc/extreme_set.cpp, gs_compact_offsets), through
its pure-host debug entry.

The sorter decides from the EXTREME SET of the centres, which holds every hull vertex, so the per-axis min and max over the set are
those over all centres.  Here the set comes from gs_debug_extreme_set (test_extreme_set.extreme_set) and the verdict and the offsets
are compared with brute force over ALL points in numpy int64: fits <=> max - min <= 65535 on every axis, offset = the minimum."""
import ctypes as C

import numpy as np
import pytest

import gaussiansplats3d_amd as g
from test_extreme_set import extreme_set


def compact_offsets(rows3):
    """rows3: (n, 3) integers.  Returns (fits, offsets as a tuple or None)."""
    fn = g.load().gs_debug_compact_offsets
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    p = np.asarray(rows3, dtype=np.int64).reshape(-1, 3)
    a = np.full((len(p), 4), -123456789, dtype=np.int32)      # (the w lane is ignored)
    a[:, :3] = p
    a = np.ascontiguousarray(a)
    off = np.full(3, 0x5A5A5A5A, dtype=np.int32)
    st = fn(a.ctypes.data if len(a) else None, len(a), off.ctypes.data)
    assert st in (0, 1), st
    if st == 0:
        assert (off == 0x5A5A5A5A).all(), "a refusal leaves the offsets alone"
        return False, None
    return True, tuple(int(v) for v in off)


def brute(points):
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return bool(((hi - lo) <= 65535).all()), tuple(int(v) for v in lo)


def check(points, prior_points=None):
    """The verdict over the extreme set of `points` (extended from the set of prior_points) against brute force over all of them."""
    prior = extreme_set(prior_points) if prior_points is not None else None
    cset = extreme_set(points, prior=prior)
    assert cset is not None
    everything = points if prior_points is None else np.concatenate([prior_points, points])
    fits, lo = brute(everything)
    got, off = compact_offsets(cset)
    assert got == fits
    if fits:
        assert off == lo
    return got


def clouds():
    rng = np.random.default_rng(77)
    n = 3000
    return {
        "gaussian blob": np.rint(rng.normal(size=(n, 3)) * 3000).astype(np.int64),
        "the C3 stand-in's box": rng.integers(-8000, 8001, size=(n, 3)),
        "wide blob": np.rint(rng.normal(size=(n, 3)) * 30000).astype(np.int64),
        "box just inside": rng.integers(-32768, 32768, size=(n, 3)),
        "negative corner": rng.integers(-2_000_000, -1_950_000, size=(n, 3)),
        "near +2^20": rng.integers((1 << 20) - 500, (1 << 20) + 500, size=(n, 3)),
        "one wide axis": np.stack([rng.integers(0, 100, size=n), rng.integers(-70000, 70000, size=n), rng.integers(0, 100, size=n)], axis=1),
        "all equal": np.tile(np.array([[5, -6, 7]], dtype=np.int64), (n, 1)),
        "one point": np.array([[-9, 8, 7]], dtype=np.int64),
        "line": np.array([(3 * i - 7, -5 * i, 11 * i) for i in range(n)], dtype=np.int64),
    }


CLOUDS = clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_random_clouds_against_brute_force(name):
    fits = check(CLOUDS[name])
    if name in ("wide blob", "one wide axis"):
        assert not fits
    if name in ("gaussian blob", "the C3 stand-in's box", "box just inside", "negative corner", "near +2^20", "all equal", "one point"):
        assert fits


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("base", [-40000, 0, (1 << 20) - 7, -(1 << 31), (1 << 31) - 1 - 65536])
def test_an_extent_of_65535_fits_and_65536_does_not(axis, base):
    rng = np.random.default_rng(axis + 3)
    pts = rng.integers(-1000, 1001, size=(500, 3)).astype(np.int64)
    pts[:, axis] = base + rng.integers(0, 65536, size=500)
    pts[0, axis], pts[1, axis] = base, base + 65535
    assert check(pts) is True
    pts[1, axis] = base + 65536
    assert check(pts) is False


def test_centres_at_the_int32_limits():
    lo, hi = -(1 << 31), (1 << 31) - 1
    rng = np.random.default_rng(9)
    assert check(np.array([[lo, lo, lo], [hi, hi, hi]], dtype=np.int64)) is False        # hi - lo = 2^32 - 1: int64 arithmetic
    assert check(np.array([[lo, 0, hi], [lo + 65535, 65535, hi - 65535]], dtype=np.int64)) is True
    assert check(np.array([[lo, 0, hi], [lo + 65535, 65535, hi - 65536]], dtype=np.int64)) is False
    top = hi - rng.integers(0, 65536, size=(800, 3))
    assert check(top) is True
    bottom = lo + rng.integers(0, 65536, size=(800, 3))
    assert check(bottom) is True
    assert check(rng.integers(lo, hi + 1, size=(800, 3))) is False


def test_zero_filled_slots_count_as_the_origin():
    """gs_sorter_set_uploaded_count adds the point (0, 0, 0) to the set: a scene away from the origin stops fitting, or moves its
    offsets, exactly as brute force over the centres plus the origin says."""
    rng = np.random.default_rng(12)
    origin = np.zeros((1, 3), dtype=np.int64)
    near = rng.integers(2000, 30000, size=(1500, 3))
    assert check(near) is True
    assert check(origin, prior_points=near) is True                                      # the offsets drop to 0
    far = rng.integers(70000, 90000, size=(1500, 3))
    assert check(far) is True
    assert check(origin, prior_points=far) is False
    straddle = rng.integers(-30000, 30000, size=(1500, 3))
    assert check(origin, prior_points=straddle) is True                                  # the origin is inside: nothing moves


def test_appended_ranges_decide_like_a_rebuild():
    rng = np.random.default_rng(13)
    a = rng.integers(-5000, 5000, size=(1200, 3))
    b = rng.integers(20000, 40000, size=(1200, 3))
    c = rng.integers(60000, 61000, size=(1200, 3))
    assert check(b, prior_points=a) is True
    assert check(c, prior_points=np.concatenate([a, b])) is False


def test_no_rows_do_not_fit():
    assert compact_offsets(np.zeros((0, 3), dtype=np.int64)) == (False, None)
