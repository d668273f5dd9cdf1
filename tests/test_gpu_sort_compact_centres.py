"""-m gpu: 16-bit offset centre planes for the known-range front end.  A static integer sorter whose extreme set spans at most 65535
per axis keeps c - o (o = the per-axis minimum) as three uint16 planes, and k_depth_key_hist<true, true> keys the identity list from
them: K0 + dx * im0 + dy * im1 + dz * im2 in uint32, K0 = im . o, which is im . c mod 2^32 bit for bit.

Every sort is held bit for bit to the sort oracle by known_range_cases.check_sort - the list, the keys (debug_read 0: rebuilt from
the int32 planes), the buckets (debug_read 1), key_min / key_max / clamped, the front end (debug_read 4) - and word 7 of
debug_read 4 says whether the front end read the 16-bit planes.  GSPLAT_NO_COMPACT_CENTRES is read once per process: that variant
runs this file as a child process (`python test_gpu_sort_compact_centres.py GSPLAT_NO_COMPACT_CENTRES`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import known_range_cases as K
from known_range_cases import KNOWN, OLD
from gaussiansplats3d_amd import Context, create_sort_worker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHUNK = 12288                                                 # keys of one scatter chunk; a vector is 8 positions
# the scalar path alone, one vector - 1 / exactly / + 1, one chunk - 1 / exactly / + 1, three chunks + 5, several workgroups
SIZES = (1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 100003)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def compact_word(w):
    return int(w.debug_read(4, 8)[7])


def worker_with(ctx, centers4, capacity=None, **kw):
    w = create_sort_worker(ctx, capacity or centers4.shape[0], **kw)
    K.upload(w, centers4)
    return w


def check(w, centers4, mvp, compact, path=KNOWN, what="", **kw):
    sel = K.check_sort(w, centers4, mvp, path, what=what, **kw)
    assert compact_word(w) == compact, f"{what}: word 7 = {compact_word(w)}, expected {compact}"
    return sel


def span_axis(ci, axis, lo, extent):
    """Makes axis `axis` of ci span exactly [lo, lo + extent]: every value folded into it, the two ends set (at positions that are
    no hull vertex of the other axes by construction of the callers' clouds)."""
    ci[:, axis] = lo + (ci[:, axis].astype(np.int64) - lo) % (extent + 1)
    ci[len(ci) // 3, axis] = lo
    ci[2 * len(ci) // 3, axis] = lo + extent


@pytest.mark.parametrize("n", SIZES)
def test_compact_sorts_match_the_oracle(ctx, n):
    ci = K.gaussian_centers(n, seed=1000 + n)                 # negative and positive coordinates, about +-12000
    if n > 1:
        assert ci[:, :3].min() < 0 < ci[:, :3].max()
    w = worker_with(ctx, ci)
    for k in (0, 1):
        check(w, ci, K.camera_mvp(k), 1, what=f"n {n} camera {k}")
    w.terminate()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_an_extent_of_65535_is_compact_and_65536_is_not(ctx, axis):
    n = CHUNK + 1
    ci = K.gaussian_centers(n, seed=40 + axis, offset=(-20000, 5000, 30000))
    span_axis(ci, axis, -41000, 65535)
    assert int(ci[:, axis].max()) - int(ci[:, axis].min()) == 65535
    w = worker_with(ctx, ci)
    check(w, ci, K.camera_mvp(axis), 1, what="extent 65535")
    w.terminate()
    span_axis(ci, axis, -41000, 65536)
    assert int(ci[:, axis].max()) - int(ci[:, axis].min()) == 65536
    w = worker_with(ctx, ci)
    check(w, ci, K.camera_mvp(axis), 0, what="extent 65536")
    w.terminate()


def test_an_offset_whose_key_wraps_while_no_real_key_does(ctx):
    """Centres near (+2^20, -2^20) on a thin diagonal, x + y ~ 0: with im = (40000, 40000, 3000) every real key is small, but the
    offset o = (min x, min y, min z) is a corner far off the diagonal and im . o leaves int32.  The device adds im . (c - o) to the
    wrapped K0 and must land on the real key: linear mod 2^32."""
    n = 3 * CHUNK + 5
    rng = np.random.default_rng(5)
    t = rng.integers(0, 60001, size=n)
    ci = np.empty((n, 4), dtype=np.int32)
    ci[:, 0] = (1 << 20) + t + rng.integers(-40, 41, size=n)
    ci[:, 1] = -(1 << 20) - t + rng.integers(-40, 41, size=n)
    ci[:, 2] = rng.integers(-900, 901, size=n)
    ci[:, 3] = 1000
    ci[0, :2], ci[1, :2] = ((1 << 20), -(1 << 20)), ((1 << 20) + 60000, -(1 << 20) - 60000)
    mvp = K.camera_mvp(0).copy()
    mvp[[2, 6, 10]] = (40.0, 40.0, 3.0)
    im = (40000, 40000, 3000)
    o = [int(ci[:, k].min()) for k in range(3)]
    k0 = sum(a * b for a, b in zip(im, o))
    keys = ci[:, :3].astype(np.int64) @ np.array(im, dtype=np.int64)
    assert not -(1 << 31) <= k0 < (1 << 31), "the offset's key was meant to wrap"
    assert -(1 << 31) <= keys.min() and keys.max() < (1 << 31)
    assert all(int(ci[:, k].max()) - o[k] <= 65535 for k in range(3))
    w = worker_with(ctx, ci)
    check(w, ci, mvp, 1, what="K0 wraps")
    mvp[[2, 6, 10]] = (-40.0, -40.0, 3.0)                      # ... and through the other end of int32
    check(w, ci, mvp, 1, what="K0 wraps negative im")
    w.terminate()
    # the same cloud at the other sign, a small extent near -2^20 / +2^20
    cj = ci.copy()
    cj[:, :2] = -ci[:, :2]
    w = worker_with(ctx, cj)
    mvp[[2, 6, 10]] = (40.0, 40.0, 3.0)
    check(w, cj, mvp, 1, what="K0 wraps, mirrored")
    check(w, cj, K.camera_mvp(2), 1, what="an ordinary camera far from the origin")
    w.terminate()


def test_all_centres_equal(ctx):
    n = 5003
    same = np.tile(np.array([[1234, -567, 89, 1000]], dtype=np.int32), (n, 1))
    w = worker_with(ctx, same)
    sel = check(w, same, K.camera_mvp(0), 1, what="all centres equal")        # every offset plane is zero, every key is K0
    assert sel[1] == 1 and sel[2] == sel[3]
    w.terminate()


def test_the_lifecycle_of_the_planes(ctx):
    """Appended ranges, an overwrite out of and back into 16 bits, an offset that moves, a zero-filled tail."""
    n0, n1, n2 = 20003, 9001, 4099
    cap = n0 + n1 + n2 + 50
    a = K.gaussian_centers(n0, seed=60, scale=2500)
    w = worker_with(ctx, a, capacity=cap)
    check(w, a, K.camera_mvp(0), 1, what="first upload")
    b = K.gaussian_centers(n1, seed=61, scale=1500, offset=(3000, -2000, 1000))   # inside the first range's box
    ab = np.concatenate([a, b])
    K.upload(w, ab, n0, n0 + n1)
    check(w, ab, K.camera_mvp(1), 1, what="an appended range that keeps the extent")
    c = K.gaussian_centers(n2, seed=62, scale=300, offset=(0, 90000, 0))           # y now spans more than 2^16
    abc = np.concatenate([ab, c])
    K.upload(w, abc, n0 + n1, n0 + n1 + n2)
    check(w, abc, K.camera_mvp(2), 0, what="an appended range past 16 bits")
    abc = abc.copy()
    abc[n0 + n1:] = K.gaussian_centers(n2, seed=63, scale=300, offset=(0, 9000, 0))
    K.upload(w, abc, n0 + n1, n0 + n1 + n2)
    check(w, abc, K.camera_mvp(3), 1, what="overwritten back into 16 bits")
    lo_before = abc[:, :3].min(axis=0)
    abc = abc.copy()
    abc[7, :3] = lo_before - (5000, 1, 7000)                   # a new minimum on every axis: all three offsets move
    assert ((abc[:, :3].max(axis=0).astype(np.int64) - abc[:, :3].min(axis=0)) <= 65535).all()
    K.upload(w, abc, 0, 16)
    check(w, abc, K.camera_mvp(4), 1, what="the offsets moved")
    check(w, abc, K.camera_mvp(5), 1, what="the offsets moved, next camera")
    w.set_uploaded_count(cap)                                  # 50 zero-filled slots: the origin is inside the box
    grown = np.concatenate([abc, np.zeros((50, 4), dtype=np.int32)])
    check(w, grown, K.camera_mvp(6), 1, what="zero-filled tail")
    w.terminate()
    # a scene far from the origin: its zero-filled tail widens x past 16 bits
    far = K.gaussian_centers(5003, seed=64, scale=300, offset=(80000, 100, -100))
    w = worker_with(ctx, far, capacity=5003 + 9)
    check(w, far, K.camera_mvp(0), 1, what="far scene")
    w.set_uploaded_count(5003 + 9)
    check(w, np.concatenate([far, np.zeros((9, 4), dtype=np.int32)]), K.camera_mvp(1), 0, what="far scene with a zero-filled tail")
    w.terminate()


def test_the_int32_keys_are_rebuilt_after_a_compact_sort(ctx):
    """Selectors 0 and 1 describe the sort that ran: its depths are rebuilt from the int32 planes, which the compact path left alone."""
    import oracle
    n = CHUNK + 1
    ci = K.gaussian_centers(n, seed=70, offset=(-7000, 300, 12000))
    w = worker_with(ctx, ci)
    for k in (0, 1):
        w.post_message({"sort": {"modelViewProj": K.camera_mvp(k), "splatRenderCount": n, "splatSortCount": n, "usePrecomputedDistances": False,
                                 "indexesToSort": None, "transforms": None, "precomputedDistances": None}})
    assert w.debug_read(4, 8).tolist()[6:] == [1, 1]
    _, keys, buckets, _, _ = oracle.sort_indexes(np.arange(n, dtype=np.uint32), ci, K.camera_mvp(1), return_intermediates=True)
    np.testing.assert_array_equal(w.debug_read(0, n), keys)
    np.testing.assert_array_equal(w.debug_read(1, n), buckets)
    check(w, ci, K.camera_mvp(2), 1, what="a compact sort after the rebuilt keys")
    w.terminate()


def test_every_other_sort_reads_the_int32_planes(ctx):
    n = 20003
    ci = K.gaussian_centers(n, seed=80)
    rng = np.random.default_rng(81)
    w = worker_with(ctx, ci)
    check(w, ci, K.camera_mvp(0), 1)
    check(w, ci, K.camera_mvp(1), 0, path=OLD, sort_count=n // 2, what="partial")
    check(w, ci, K.camera_mvp(2), 0, path=OLD, indexes=rng.permutation(n).astype(np.uint32), what="host index list")
    check(w, ci, K.camera_mvp(3), 1)
    w.terminate()
    w = worker_with(ctx, ci, splat_sort_distance_map_precision=20)
    check(w, ci, K.camera_mvp(0), 0, precision=20, what="20-bit buckets: int32 keys from int32 planes")
    w.terminate()
    # words 0 .. 6 of selector 4 are what they were: a read of 6 or 7 words is a prefix of the read of 8
    w = worker_with(ctx, ci)
    check(w, ci, K.camera_mvp(4), 1)
    full = w.debug_read(4, 8).tolist()
    assert w.debug_read(4, 6).tolist() == full[:6] and w.debug_read(4, 7).tolist() == full[:7]
    w.terminate()


def run_child(mode):
    """GSPLAT_NO_COMPACT_CENTRES, read once per process.  Prints one JSON line."""
    assert mode == "GSPLAT_NO_COMPACT_CENTRES"
    import zlib
    ctx = Context(0)
    done = {}
    for n in (9, CHUNK + 1, 100003):
        ci = K.gaussian_centers(n, seed=1000 + n)
        w = create_sort_worker(ctx, n)
        K.upload(w, ci)
        for k in (0, 1):
            K.check_sort(w, ci, K.camera_mvp(k), KNOWN, what=mode)
            assert w.debug_read(4, 8).tolist()[6:] == [1, 0], f"{mode} n {n}: {w.debug_read(4, 8).tolist()}"
        done[str(n)] = zlib.crc32(w.debug_read(2, n).tobytes())
        w.terminate()
    ctx.close()
    print(json.dumps({"done": done}))


def test_the_switch_in_a_process_of_its_own(ctx):
    """GSPLAT_NO_COMPACT_CENTRES=1 restores the int32 reads: word 7 = 0, 16-bit keys as before, the same lists."""
    env = dict(os.environ)
    env["GSPLAT_NO_COMPACT_CENTRES"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([HERE, ROOT, env.get("PYTHONPATH", "")])
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "GSPLAT_NO_COMPACT_CENTRES"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    theirs = json.loads(run.stdout.strip().splitlines()[-1])["done"]
    assert len(theirs) == 3
    import zlib
    for n, crc in theirs.items():
        n = int(n)
        ci = K.gaussian_centers(n, seed=1000 + n)
        w = worker_with(ctx, ci)
        check(w, ci, K.camera_mvp(1), 1, what="the same sort in this process")
        assert zlib.crc32(w.debug_read(2, n).tobytes()) == crc, f"n {n}: the list differs from the int32 path's"
        w.terminate()


if __name__ == "__main__":
    run_child(sys.argv[1])
