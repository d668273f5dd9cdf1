"""Shared by tests/test_gpu_sort_known_range.py and its child processes: one sort through the SortWorker, held bit for bit to the
sort oracle - the sorted list, the keys (debug_read 0), the buckets (debug_read 1), key_min / key_max / clamped - and to the path
the test means to exercise (debug_read 4: {known-range front end, |extreme set|, lo, hi, set valid, pass 0's slot})."""
import json
import sys

import numpy as np

import oracle
from gaussiansplats3d_amd import camera, create_sort_worker

KNOWN, OLD = "known", "old"


def gaussian_centers(n, seed, scale=3000.0, offset=(0, 0, 0)):
    """int32 [n, 4] centres as the Viewer posts them (x1000 integers, w = 1000)."""
    rng = np.random.default_rng(seed)
    c = np.empty((n, 4), dtype=np.int32)
    c[:, :3] = np.rint(rng.normal(size=(n, 3)) * scale).astype(np.int32) + np.asarray(offset, dtype=np.int32)
    c[:, 3] = 1000
    return c


def camera_mvp(k=0):
    """A few different cameras: the demo pose, turned about the vertical axis."""
    m = np.asarray(camera.demo_camera("garden", 640, 360).sort_mvp(), dtype=np.float64).reshape(4, 4, order="F")
    a = 0.7 * k
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    return (m @ rot).reshape(16, order="F")


def expected_clamps(keys, lo, hi, precision):
    """Buckets outside [0, range) before the clamp (sorter.cpp:142-146 in fp32), from the oracle's keys and range."""
    if len(keys) == 0 or hi == lo:
        return 0                                              # NaN range map: every bucket is 0, none is clamped
    rng = 1 << precision
    range_map = np.float32(rng - 1) / (np.float32(hi) - np.float32(lo))
    diff = ((keys.astype(np.int64) - lo) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    f = diff.astype(np.float32) * range_map
    fits = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    b = np.where(fits, np.trunc(np.where(fits, f, 0)), 0).astype(np.int64)
    return int(((b < 0) | (b >= rng)).sum())


def check_sort(w, centers4, mvp, path, sort_count=None, render_count=None, indexes=None, precision=16, use_int=True, dynamic=False,
               scene_indexes=None, transforms=None, precomputed=None, uploaded=None, what=""):
    """One sort of `w` (which holds centers4) against the oracle; returns debug_read(4).  use_int = False: fp32 centres (or
    distances); precomputed: one distance per uploaded splat; uploaded: the sorter's count where centers4 is longer (only the
    listed rows of centers4 are read)."""
    n = centers4.shape[0] if uploaded is None else uploaded
    R = n if render_count is None else render_count
    Rs = R if sort_count is None else sort_count
    reply = w.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": R, "splatSortCount": Rs,
                                     "usePrecomputedDistances": precomputed is not None, "indexesToSort": indexes, "transforms": transforms,
                                     "precomputedDistances": precomputed}})
    idx = np.arange(n, dtype=np.uint32) if indexes is None else indexes
    exp, keys, buckets, (lo, hi), st = oracle.sort_indexes(idx, centers4, mvp, sort_count=Rs, render_count=R, precision=precision,
                                                          use_int=use_int, dynamic=dynamic, precomputed=precomputed,
                                                          scene_indexes=scene_indexes, transforms=transforms, return_intermediates=True)
    tag = f"{what} n {n} R {R} Rs {Rs}"
    sel = w.debug_read(4, 6)
    assert sel[0] == (1 if path == KNOWN else 0), f"{tag}: front end {sel.tolist()}, expected the {path} path"
    np.testing.assert_array_equal(reply["sortedIndexes"], exp, err_msg=tag)
    s0 = R - Rs
    np.testing.assert_array_equal(w.debug_read(0, R)[s0:], keys[s0:], err_msg=tag)
    np.testing.assert_array_equal(w.debug_read(1, R)[s0:], buckets[s0:], err_msg=tag)
    stats = reply["stats"]
    assert (stats.key_min, stats.key_max) == (lo, hi), tag
    # (integer mode: the formula above; float mode: what the oracle's own bucket map clamped)
    clamps = expected_clamps(keys[s0:], lo, hi, precision) if use_int else oracle.count_clamped(keys[s0:], lo, hi, precision)
    assert stats.clamped == clamps, f"{tag}: clamped {stats.clamped}, the oracle {clamps}"
    assert reply["status"] == st, tag
    if path == KNOWN:
        assert (int(sel[2]), int(sel[3])) == (lo, hi), f"{tag}: the host's range {sel.tolist()} against the oracle's {(lo, hi)}"
        assert sel[1] >= 1 and sel[4] == 1, tag
    return sel


def upload(w, centers4, a=0, b=None):
    b = centers4.shape[0] if b is None else b
    w.post_message({"centers": centers4[a:b], "range": {"from": a, "to": b - 1, "count": b - a}})


def run_child(mode):
    """Scenarios whose switches are read once per process.  Prints one JSON line."""
    from gaussiansplats3d_amd import Context
    ctx = Context(0)
    done = []
    if mode == "GSPLAT_NO_KNOWN_RANGE":
        sizes, path = (1, 4097, 12293, 100000), OLD
    elif mode == "GSPLAT_NO_SORT_CHUNK":
        # pass 0 is the tile kernel: one tile per workgroup, two, and chunks longer than one batch of the key kernel's loads
        sizes, path = (3, 4097, 100000, 2_100_001, 6_300_013), KNOWN
    else:
        sizes, path = (3, 4097, 12293, 100000), KNOWN           # GSPLAT_NO_SORT_PACK: key + value passes behind the known-range front end
    for n in sizes:
        ci = gaussian_centers(n, seed=n)
        w = create_sort_worker(ctx, n)
        upload(w, ci)
        for k in range(2 if n <= 100000 else 1):
            sel = check_sort(w, ci, camera_mvp(k), path, what=mode)
            if path == OLD:
                assert sel[1] == 0 and sel[4] == 0, "the switch keeps no extreme set"
        w.terminate()
        done.append(n)
    ctx.close()
    print(json.dumps({"done": done}))


if __name__ == "__main__":
    run_child(sys.argv[1])
