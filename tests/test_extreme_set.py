"""CPU tier: the extreme set of a static integer sorter's centres (csrc/extreme_set.cpp) through its pure-host debug entry.

Contract: the set is a subset of the points and holds every vertex of their convex hull, so for EVERY direction d the min and max
of d . c over the set equal the min and max over all points.  Checked exactly, in Python integers, for the six axis directions,
200 seeded random integer directions and the normals of faces spanned by triples of returned points (the directions most likely to
expose a dropped vertex).  A set that does not fit the cap is reported as "no set"."""
import ctypes as C

import numpy as np
import pytest

import gaussiansplats3d_amd as g

CAP = 4096


def _entry():
    fn = g.load().gs_debug_extreme_set
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    return fn


def extreme_set(points, prior=None, cap=CAP):
    """points, prior: (n, 3) integers.  Returns the set as an (m, 3) int64 array, or None when it does not fit the cap."""
    def rows(p):
        p = np.asarray(p, dtype=np.int64).reshape(-1, 3)
        a = np.full((len(p), 4), 77, dtype=np.int32)          # (the w lane is ignored)
        a[:, :3] = p
        return np.ascontiguousarray(a)
    a = rows(points)
    b = rows(prior) if prior is not None else np.zeros((0, 4), dtype=np.int32)
    out = np.zeros((cap, 4), dtype=np.int32)
    n = C.c_uint32(0)
    st = _entry()(b.ctypes.data if len(b) else None, len(b), a.ctypes.data if len(a) else None, len(a), cap, out.ctypes.data, C.byref(n))
    assert st in (0, 1), st
    if st == 1:
        assert n.value == 0
        return None
    assert n.value <= cap
    return out[:n.value, :3].astype(np.int64)


def _dots(points, d):
    """d . p per point in exact Python integers (coordinates near 2^31 times directions near 2^67 leave int64)."""
    return [int(p[0]) * d[0] + int(p[1]) * d[1] + int(p[2]) * d[2] for p in points]


def directions(cset, seed):
    rng = np.random.default_rng(seed)
    ds = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ds += [tuple(int(v) for v in rng.integers(-1_000_000, 1_000_001, size=3)) for _ in range(200)]
    if len(cset) >= 3:                                         # normals of faces spanned by triples of returned points
        for _ in range(60):
            i, j, k = (int(v) for v in rng.choice(len(cset), size=3, replace=False))
            u = [int(cset[j][c]) - int(cset[i][c]) for c in range(3)]
            v = [int(cset[k][c]) - int(cset[i][c]) for c in range(3)]
            n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            if any(n):
                ds += [n, (-n[0], -n[1], -n[2])]
    return ds


def check_extremes(points, cset, seed=5):
    points = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    assert cset is not None, "no set reported"
    assert len(cset) >= 1
    all_rows = {tuple(int(v) for v in p) for p in points}
    assert all(tuple(int(v) for v in p) in all_rows for p in cset), "the set is no subset of the points"
    # int64 is exact for the small directions; the face normals go through Python integers
    for d in directions(cset, seed):
        if max(abs(v) for v in d) <= 1_000_000:
            dv = np.array(d, dtype=np.int64)
            full, sub = points @ dv, cset @ dv                 # |coordinate| < 2^31, |d| <= 10^6: below 2^53
            assert int(full.min()) == int(sub.min()) and int(full.max()) == int(sub.max()), d
        else:
            full, sub = _dots(points, d), _dots(cset, d)
            assert min(full) == min(sub) and max(full) == max(sub), d


def _sphere(rng, n, radius=1_000_000):
    v = rng.normal(size=(n, 3))
    return np.rint(v / np.linalg.norm(v, axis=1, keepdims=True) * radius).astype(np.int64)


def point_sets():
    rng = np.random.default_rng(2024)
    n = 3000
    sets = {
        "gaussian blob": np.rint(rng.normal(size=(n, 3)) * 3000).astype(np.int64),
        "uniform box": rng.integers(-10_000, 10_001, size=(n, 3)),
        "planar grid": np.array([(10 * i + 3 * j, 7 * i - 2 * j, 5 * i + j) for i in range(50) for j in range(50)], dtype=np.int64),
        "axis plane": np.array([(i, j, 9) for i in range(40) for j in range(40)], dtype=np.int64),
        "line": np.array([(3 * i - 7, -5 * i, 11 * i) for i in range(n)], dtype=np.int64),
        "all equal": np.tile(np.array([[5, -6, 7]], dtype=np.int64), (n, 1)),
        "heavy duplicates": rng.integers(-3, 4, size=(n, 3)),
        "near +-2^30": (rng.choice([-1, 1], size=(n, 3)) * ((1 << 30) - rng.integers(0, 1000, size=(n, 3)))).astype(np.int64),
        "full int32 range": rng.integers(-(1 << 31), 1 << 31, size=(n, 3)),
        "small sphere under the cap": _sphere(rng, 500),
    }
    for k in range(1, 6):
        sets[f"{k} points"] = rng.integers(-100, 101, size=(k, 3))
    return sets


POINT_SETS = point_sets()


@pytest.mark.parametrize("name", sorted(POINT_SETS))
def test_the_set_holds_the_extremes_of_every_direction(name):
    pts = POINT_SETS[name]
    cset = extreme_set(pts)
    check_extremes(pts, cset)
    if name == "all equal":
        assert len(cset) == 1
    if name == "line":
        assert len(cset) == 2
    if name in ("gaussian blob", "uniform box"):
        assert len(cset) < len(pts) // 4, "the filter dropped next to nothing"


def test_points_on_a_sphere_report_the_cap():
    rng = np.random.default_rng(3)
    assert extreme_set(_sphere(rng, 6000)) is None             # every point is a hull vertex: more than the cap
    pts = _sphere(rng, 600)
    assert extreme_set(pts, cap=256) is None
    check_extremes(pts, extreme_set(pts, cap=1024))


def test_no_points_give_the_empty_set():
    cset = extreme_set(np.zeros((0, 3), dtype=np.int64))
    assert cset is not None and len(cset) == 0


def test_appended_ranges_extend_the_set_like_a_rebuild():
    rng = np.random.default_rng(11)
    parts = [np.rint(rng.normal(size=(1500, 3)) * s + o).astype(np.int64) for s, o in ((2000, 0), (500, 9000), (4000, -3000))]
    cset = None
    for k, part in enumerate(parts):
        cset = extreme_set(part, prior=cset)                   # hull(old U new) = hull(set(old) U new)
        seen = np.concatenate(parts[:k + 1])
        check_extremes(seen, cset, seed=k)
    rebuilt = extreme_set(np.concatenate(parts))
    check_extremes(np.concatenate(parts), rebuilt)
    # the zero fill of gs_sorter_set_uploaded_count adds the point (0, 0, 0)
    far = parts[1]
    grown = extreme_set(np.zeros((1, 3), dtype=np.int64), prior=extreme_set(far))
    check_extremes(np.concatenate([far, np.zeros((1, 3), dtype=np.int64)]), grown)
    # a degenerate set that grows out of its line / plane
    line = POINT_SETS["line"]
    cset = extreme_set(line)
    cset = extreme_set(np.array([[1, 1, 1]]), prior=cset)
    check_extremes(np.concatenate([line, [[1, 1, 1]]]), cset)
    cset = extreme_set(np.array([[-50, 400, 3]]), prior=cset)
    check_extremes(np.concatenate([line, [[1, 1, 1]], [[-50, 400, 3]]]), cset)


# ---------------------------------------------------------------------------------------------------------------------------
# the exact key range of a sort over the set (gs_key_range): min / max of im . c in exact integers, refused when a key could wrap
# ---------------------------------------------------------------------------------------------------------------------------
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def key_range(rows, im):
    """rows: (n, 3) integers, im: 3 integers (all int32).  (lo, hi), or None when the library reports no range."""
    a = np.full((len(rows), 4), 77, dtype=np.int32)            # (the w lane is ignored)
    if len(rows):
        a[:, :3] = np.asarray(rows, dtype=np.int64)
    im3 = np.asarray(im, dtype=np.int32)
    out = np.array([123, 456], dtype=np.int32)
    fn = g.load().gs_debug_key_range
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    st = fn(a.ctypes.data if len(rows) else None, len(rows), im3.ctypes.data, out.ctypes.data)
    assert st in (0, 1), st
    if st == 0:
        assert out.tolist() == [123, 456]                      # lo / hi are left alone
        return None
    return int(out[0]), int(out[1])


def key_range_model(rows, im):
    if not len(rows):
        return None
    v = _dots(rows, tuple(int(k) for k in im))
    return (min(v), max(v)) if min(v) >= INT32_MIN and max(v) <= INT32_MAX else None


BIG = 1 << 29
KEY_RANGE_CASES = [
    # (name, rows, im, expected or "model")
    ("empty_set", [], (1, 2, 3), None),
    ("one_row", [(5, -7, 11)], (1000, -2000, 3000), (5000 + 14000 + 33000, 52000)),
    ("zero_coefficients", [(INT32_MAX, INT32_MIN, 5), (1, 2, 3)], (0, 0, 0), (0, 0)),
    # coefficients at +-2^29: the int64 branch's largest products (3 x 2^29 x 2^31 = 3 x 2^60), far outside int32
    ("im_at_2p29_extreme_rows", [(INT32_MAX, INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MIN, INT32_MIN)], (BIG, BIG, BIG), None),
    ("im_at_minus_2p29_extreme_rows", [(INT32_MIN, INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MIN, INT32_MAX)], (-BIG, -BIG, -BIG), None),
    ("im_at_2p29_small_rows", [(1, 1, 1), (-1, -2, -1), (0, 3, 0)], (BIG, BIG, BIG), (-4 * BIG, 3 * BIG)),
    ("im_at_2p29_cancelling", [(INT32_MAX, INT32_MIN + 1, 0), (3, 0, 0)], (BIG, BIG, -BIG), (0, 3 * BIG)),
    # ... and beyond: the __int128 branch (sums reach 3 x 2^62)
    ("im_beyond_2p29_small_rows", [(1, 0, 0), (0, 0, 1), (-1, 0, 0)], (BIG + 1, 5, -7), (-(BIG + 1), BIG + 1)),
    ("im_int32_extremes_wrap", [(INT32_MIN, INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX, INT32_MAX)], (INT32_MIN, INT32_MIN, INT32_MIN), None),
    ("im_int32_max_cancelling", [(INT32_MAX, INT32_MAX, 0), (2, 1, 0)], (INT32_MAX, -INT32_MAX, 1), (0, INT32_MAX)),
    ("im_int32_min_times_one", [(1, 0, 0), (0, 0, 0)], (INT32_MIN, 0, 0), (INT32_MIN, 0)),
    ("im_int32_min_times_minus_one_is_one_beyond", [(-1, 0, 0), (0, 0, 0)], (INT32_MIN, 0, 0), None),
    # ranges that end exactly at INT32_MIN / INT32_MAX, and one beyond them - in either branch
    ("hi_at_int32_max", [(INT32_MAX, 0, 0), (0, 0, 0)], (1, 1, 1), (0, INT32_MAX)),
    ("hi_one_beyond_int32_max", [(INT32_MAX, 1, 0), (0, 0, 0)], (1, 1, 1), None),
    ("lo_at_int32_min", [(INT32_MIN, 0, 0), (0, 0, 0)], (1, 1, 1), (INT32_MIN, 0)),
    ("lo_one_beyond_int32_min", [(INT32_MIN, -1, 0), (0, 0, 0)], (1, 1, 1), None),
    ("both_ends_exact", [(INT32_MAX, 0, 0), (0, INT32_MIN, 0)], (1, 1, 0), (INT32_MIN, INT32_MAX)),
    ("hi_at_int32_max_int128", [(0, 0, INT32_MAX), (0, 0, 0)], (BIG + 5, 7, 1), (0, INT32_MAX)),
    ("hi_one_beyond_int32_max_int128", [(0, 1, INT32_MAX), (0, 0, 0)], (BIG + 5, 1, 1), None),
    ("lo_at_int32_min_int128", [(0, 0, INT32_MIN), (0, 0, 0)], (-BIG - 5, 7, 1), (INT32_MIN, 0)),
    ("lo_one_beyond_int32_min_int128", [(0, -1, INT32_MIN), (0, 0, 0)], (-BIG - 5, 1, 1), None),
    ("product_exact_2p31_minus_1_factors", [(46341, 0, 0), (0, 0, 0)], (46340, 0, 0), (0, 46341 * 46340)),
]


@pytest.mark.parametrize("name,rows,im,expected", KEY_RANGE_CASES, ids=[c[0] for c in KEY_RANGE_CASES])
def test_key_range_in_exact_integers(name, rows, im, expected):
    assert key_range_model(rows, im) == expected, "the case's own expectation against Python integers"
    assert key_range(rows, im) == expected


def test_key_range_random_rows_and_coefficients():
    """Seeded rows and coefficients of every magnitude, both branches, against Python integers."""
    rng = np.random.default_rng(29)
    seen = {True: 0, False: 0}
    for k in range(400):
        cbits, ibits = int(rng.integers(1, 32)), int(rng.integers(1, 32))
        rows = rng.integers(-(1 << cbits), 1 << cbits, size=(int(rng.integers(1, 40)), 3)).clip(INT32_MIN, INT32_MAX)
        im = rng.integers(-(1 << ibits), 1 << ibits, size=3).clip(INT32_MIN, INT32_MAX)
        want = key_range_model(rows, im)
        assert key_range(rows, im) == want, (k, im.tolist())
        seen[want is not None] += 1
    assert min(seen.values()) >= 50                            # both verdicts, often
