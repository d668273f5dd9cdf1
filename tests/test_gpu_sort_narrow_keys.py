"""-m gpu: 16-bit radix keys out of the known-range front end.  With buckets of <= 16 bits k_depth_key_hist<true> stores
key' = range - 1 - bucket at every list position (2 bytes) instead of the int32 depth, and pass 0 reads it through
DepthLoaderT<.., .., true> in all three of its forms (chunk-staged packed, tile packed, 16-bit key + value).

Every sort is held bit for bit to the sort oracle by known_range_cases.check_sort - the list, the keys (debug_read 0: rebuilt on
demand, the sort itself no longer stores them), the buckets (debug_read 1), key_min / key_max / clamped, the front end
(debug_read 4) - and word 6 of debug_read 4 says whether the sort stored 16-bit keys.  Switches are read once per process: those
variants run this file as a child process (`python test_gpu_sort_narrow_keys.py <switch>`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import known_range_cases as K
import oracle
from known_range_cases import KNOWN, OLD
from gaussiansplats3d_amd import Context, SplatMesh, create_sort_worker, util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# Scalar path only (fewer than one aligned vector); one tile + 1; one and two chunks of CHUNK_KEYS = 12288 plus a ragged tail -
# n is odd, so the reversed 16-bit reads start at an odd element and the front end's vector cut has a head and a tail; 100 003.
SIZES = (1, 3, 5, 4097, 12289, 24579, 100003)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def narrow_word(w):
    return int(w.debug_read(4, 7)[6])


def worker_with(ctx, centers4, **kw):
    w = create_sort_worker(ctx, centers4.shape[0], **kw)
    K.upload(w, centers4)
    return w


def sort_only(w, mvp, n):
    return w.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n, "usePrecomputedDistances": False,
                                    "indexesToSort": None, "transforms": None, "precomputedDistances": None}})


@pytest.mark.parametrize("precision", [16, 10])
@pytest.mark.parametrize("n", SIZES)
def test_sorts_with_16_bit_keys_match_the_oracle(ctx, n, precision):
    ci = K.gaussian_centers(n, seed=n)
    w = worker_with(ctx, ci, splat_sort_distance_map_precision=precision)
    for k in (0, 1):
        K.check_sort(w, ci, K.camera_mvp(k), KNOWN, precision=precision, what=f"precision {precision} camera {k}")
        assert narrow_word(w) == 1
    w.terminate()


def test_20_bit_buckets_keep_the_int32_keys(ctx):
    n = 12289
    ci = K.gaussian_centers(n, seed=20)
    w = worker_with(ctx, ci, splat_sort_distance_map_precision=20)
    for k in (0, 1):
        K.check_sort(w, ci, K.camera_mvp(k), KNOWN, precision=20)
        assert narrow_word(w) == 0
    w.terminate()


def test_a_degenerate_range(ctx):
    """Five identical centres: hi == lo, the range map is NaN, every bucket is 0 - whichever front end the planner takes."""
    same = np.tile(np.array([[1234, -567, 89, 1000]], dtype=np.int32), (5, 1))
    w = worker_with(ctx, same)
    sort_only(w, K.camera_mvp(0), 5)
    path = KNOWN if int(w.debug_read(4, 6)[0]) else OLD
    sel = K.check_sort(w, same, K.camera_mvp(0), path, what="five equal centres")      # (the list, the buckets and `clamped`)
    assert narrow_word(w) == int(sel[0])
    np.testing.assert_array_equal(w.debug_read(1, 5), np.zeros(5, dtype=np.int32))
    w.terminate()


@pytest.mark.parametrize("n", [4097, 12289])
def test_a_bound_mesh_gets_its_positions_and_the_host_its_indexes(ctx, n):
    """Payloads are map[i], positions in the mesh's storage order; the host-visible list is the oracle's."""
    scene = helpers.small_scene(n, 0, seed=n)
    ci = util.integer_centers(scene.centers)
    mesh = SplatMesh(ctx, n, 0).build(scene.centers, scene.cov, scene.rgba, None)
    w = worker_with(ctx, ci)
    mesh.use_sorter_result(w, n)                              # binds
    for k in (0, 1):
        K.check_sort(w, ci, K.camera_mvp(k), KNOWN, what=f"bound mesh camera {k}")
        assert narrow_word(w) == 1
    w.terminate()
    mesh.dispose()


def test_the_selectors_describe_the_sort_that_ran(ctx):
    """`keys` is stale after a sort with 16-bit keys: selectors 0 and 1 rebuild it with that sort's coefficients."""
    n = 12289
    ci = K.gaussian_centers(n, seed=70)
    idx = np.arange(n, dtype=np.uint32)
    w = worker_with(ctx, ci)
    sort_only(w, K.camera_mvp(0), n)
    sort_only(w, K.camera_mvp(1), n)
    assert narrow_word(w) == 1
    _, keys1, buckets1, _, _ = oracle.sort_indexes(idx, ci, K.camera_mvp(1), return_intermediates=True)
    np.testing.assert_array_equal(w.debug_read(0, n), keys1)
    np.testing.assert_array_equal(w.debug_read(1, n), buckets1)
    np.testing.assert_array_equal(w.debug_read(0, n), keys1)           # twice in a row: the same answer
    # an upload between the sort and the read: still the keys of the sort that ran
    sort_only(w, K.camera_mvp(2), n)
    _, keys2, buckets2, _, _ = oracle.sort_indexes(idx, ci, K.camera_mvp(2), return_intermediates=True)
    other = K.gaussian_centers(n, seed=71, scale=900.0, offset=(500, -300, 200))
    K.upload(w, other)
    np.testing.assert_array_equal(w.debug_read(0, n), keys2)
    np.testing.assert_array_equal(w.debug_read(1, n), buckets2)
    K.check_sort(w, other, K.camera_mvp(3), KNOWN, what="after the upload")
    assert narrow_word(w) == 1
    w.terminate()


def run_child(mode):
    """One switch, read once per process.  Prints one JSON line."""
    ctx = Context(0)
    done = []
    narrow = 0 if mode == "GSPLAT_NO_NARROW_KEYS" else 1
    sizes = (3, 4097, 12289, 100003)
    if mode == "GSPLAT_NO_SORT_CHUNK":
        sizes += (2_100_001,)                                 # long chunks of the tile kernel
    for n in sizes:
        ci = K.gaussian_centers(n, seed=n)
        w = create_sort_worker(ctx, n)
        K.upload(w, ci)
        for k in range(2 if n <= 100003 else 1):
            K.check_sort(w, ci, K.camera_mvp(k), KNOWN, what=mode)
            assert narrow_word(w) == narrow, f"{mode} n {n}: word 6 = {narrow_word(w)}"
        w.terminate()
        done.append(n)
    ctx.close()
    print(json.dumps({"done": done}))


@pytest.mark.parametrize("switch", ["GSPLAT_NO_NARROW_KEYS", "GSPLAT_NO_SORT_CHUNK", "GSPLAT_NO_SORT_PACK"])
def test_switches_in_a_process_of_their_own(switch):
    """GSPLAT_NO_NARROW_KEYS keeps the int32 keys (word 6 = 0, the same lists); the two older switches change pass 0 - the tile
    kernel, 16-bit key + value output - with the 16-bit keys on (word 6 = 1)."""
    env = dict(os.environ)
    env[switch] = "1"
    env["PYTHONPATH"] = os.pathsep.join([HERE, ROOT, env.get("PYTHONPATH", "")])
    run = subprocess.run([sys.executable, os.path.abspath(__file__), switch], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert len(json.loads(run.stdout.strip().splitlines()[-1])["done"]) >= 4


if __name__ == "__main__":
    run_child(sys.argv[1])
