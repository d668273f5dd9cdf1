"""-m gpu: gpuAcceleratedSort's distance pass (gs_mesh_compute_distances = SplatMesh.computeDistancesOnGPU, SplatMesh.js:1701-1814,
shader :1449-1490) against the numpy restatement (tests/distance_cases.py), bit for bit, in all four permutations, for both storage
layouts of a mesh; and the sort of those distances through three routes - host `precomputed`, the device hand-over
(dst + GS_PRECOMPUTED_DEVICE) and the C oracle - giving identical lists."""
import ctypes as C

import numpy as np
import pytest

import oracle
from distance_cases import js_integer_centers, shader_distances, shim_centers
from gaussiansplats3d_amd import Context, SplatMesh, SplatTree, _lib as L, camera, util
from gaussiansplats3d_amd.sort_worker import SortWorker

pytestmark = pytest.mark.gpu
PERMS = [(True, False), (True, True), (False, False), (False, True)]    # (integer, dynamic)
C3_SPLATS = 5_800_000


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def scene_transforms():
    ts = []
    for k, (tx, ty, tz, s) in enumerate([(0.0, 0.0, 0.0, 1.0), (3.5, -1.25, 2.0, 0.5), (-7.0, 4.0, -2.5, 2.0)]):
        a = 0.3 * k
        m = np.eye(4)
        m[:3, :3] = s * np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        m[:3, 3] = [tx, ty, tz]
        ts.append(m.T.reshape(16))                                       # column-major
    return ts


def make_centers(n, seed, overflow=False):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-30.0, 30.0, (n, 3)).astype(np.float32)
    half = rng.random(n) < 0.05
    c[half] = np.round(c[half] * 2000.0) / 2000.0                       # x1000 lands on (or next to) Math.round's half-way points
    if overflow and n >= 8:                                              # beyond int32 after x1000, and non-finite centres
        k = rng.choice(n, size=max(4, n // 50), replace=False)
        c[k] = rng.uniform(-4e7, 4e7, (k.size, 3)).astype(np.float32)
        c[k[0]] = [np.nan, np.inf, -np.inf]
        c[k[1]] = [2147483.75, -2147483.75, 3.0e38]
    return c


def build_mesh(ctx, n, keep_order, centers, scenes, upload_split=None):
    m = SplatMesh(ctx, n, keep_order=keep_order, dynamic_mode=True)
    cov = np.zeros((n, 6), np.float32)
    rgba = np.zeros((n, 4), np.uint8)
    cuts = [0, n] if upload_split is None else [0, upload_split, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        m.build(centers[a:b], cov[a:b], rgba[a:b], start=a, scene_indexes=scenes[a:b])
    m.set_scenes(transforms=scene_transforms())
    return m


def mvp_for(seed):
    cam = camera.demo_camera("garden", 640, 360)
    mvp = np.asarray(cam.sort_mvp(), np.float64).reshape(16).copy()
    mvp[[2, 6, 10, 14]] *= 1.0 + 0.01 * seed
    return mvp


def padded_centers(centers):
    """The padFour centres the JS drop-in's own getIntegerCenters / getFloatCenters make of `centers` (the shader's inputs in the
    reference); without Node, the restatement that tests/test_distances_uniforms.py pins to them."""
    shim = shim_centers(centers)
    return shim if shim is not None else (js_integer_centers(centers), util.float_centers(centers))


def expected(centers, scenes, mvp, integer, dynamic, padded=None):
    uniforms, _ = util.distance_uniforms(mvp, integer, dynamic, scene_transforms())
    ci, cf = padded_centers(centers) if padded is None else padded
    return shader_distances(ci if integer else cf, uniforms, integer, dynamic, scenes)


def device_distances(m, mvp, integer, dynamic, n):
    out = np.full(n, -7, dtype=np.int32 if integer else np.float32)
    m.compute_distances_on_gpu(mvp, out=out, integer=integer, dynamic=dynamic)
    return out


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
@pytest.mark.parametrize("n", [1, 255, 257, 100_003, C3_SPLATS])
def test_distances_bit_exact(ctx, n, keep_order):
    centers = make_centers(n, seed=n, overflow=True)
    scenes = (np.arange(n, dtype=np.uint32) * 7 // 5) % 3
    m = build_mesh(ctx, n, keep_order, centers, scenes)
    padded = padded_centers(centers)
    for k, (integer, dynamic) in enumerate(PERMS):
        mvp = mvp_for(k)
        got = device_distances(m, mvp, integer, dynamic, n)
        want = expected(centers, scenes if dynamic else None, mvp, integer, dynamic, padded)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, keep_order, integer, dynamic)
    m.dispose()


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
def test_incremental_upload(ctx, keep_order):
    n, first = 100_003, 40_001
    centers = make_centers(n, seed=3, overflow=True)
    scenes = (np.arange(n, dtype=np.uint32) // 1000) % 3
    m = SplatMesh(ctx, n, keep_order=keep_order, dynamic_mode=True)
    cov, rgba = np.zeros((n, 6), np.float32), np.zeros((n, 4), np.uint8)
    m.build(centers[:first], cov[:first], rgba[:first], scene_indexes=scenes[:first])
    m.set_scenes(transforms=scene_transforms())
    ci, cf = padded_centers(centers)
    for k, (integer, dynamic) in enumerate(PERMS):
        got = device_distances(m, mvp_for(k), integer, dynamic, first)
        want = expected(centers[:first], scenes[:first] if dynamic else None, mvp_for(k), integer, dynamic, (ci[:first], cf[:first]))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    m.build(centers[first:], cov[first:], rgba[first:], start=first, scene_indexes=scenes[first:])   # from > 0
    for k, (integer, dynamic) in enumerate(PERMS):
        got = device_distances(m, mvp_for(k), integer, dynamic, n)
        want = expected(centers, scenes if dynamic else None, mvp_for(k), integer, dynamic, (ci, cf))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    m.dispose()


def _sort_three_ways(ctx, m, centers, scenes, mvp, integer, dynamic, n, sort_count, indexes=None):
    host = device_distances(m, mvp, integer, dynamic, n)
    tr = np.tile(np.eye(4, dtype=np.float32).reshape(16), L.GS_MAX_SCENES)
    msg = {"modelViewProj": mvp, "splatRenderCount": n if indexes is None else indexes.size, "splatSortCount": sort_count,
           "usePrecomputedDistances": True, "indexesToSort": indexes, "transforms": tr}
    lists = []
    for on_device in (False, True):
        w = SortWorker(ctx, n, integer, dynamic)
        w.set_uploaded_count(n)
        if on_device:
            m.compute_distances_on_gpu(mvp, sort_worker=w, integer=integer, dynamic=dynamic)
            reply = w.post_message({"sort": dict(msg, precomputedOnDevice=True)})
        else:
            reply = w.post_message({"sort": dict(msg, precomputedDistances=host)})
        assert reply["status"] == 0
        lists.append(reply["sortedIndexes"].copy())
        w.terminate()
    idx = np.arange(n, dtype=np.uint32) if indexes is None else indexes
    c4 = js_integer_centers(centers) if integer else util.float_centers(centers)
    lists.append(oracle.sort_indexes(idx, c4, np.asarray(mvp, np.float64).astype(np.float32), sort_count=sort_count,
                                     render_count=idx.size, use_int=integer, dynamic=dynamic, precomputed=host,
                                     scene_indexes=scenes, transforms=tr))
    return host, lists


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
@pytest.mark.parametrize("n", [257, 100_003])
def test_three_sort_routes_agree(ctx, n, keep_order):
    centers = make_centers(n, seed=11 + n)
    scenes = (np.arange(n, dtype=np.uint32) * 3 // n).astype(np.uint32)
    m = build_mesh(ctx, n, keep_order, centers, scenes)
    rng = np.random.default_rng(5)
    for k, (integer, dynamic) in enumerate(PERMS):
        mvp = mvp_for(k)
        for sort_count, indexes in ((n, None), (n // 3, None), (n // 2, rng.permutation(n)[: n - 17].astype(np.uint32))):
            host, lists = _sort_three_ways(ctx, m, centers, scenes, mvp, integer, dynamic, n, sort_count, indexes)
            assert np.array_equal(lists[0], lists[2]), ("host", integer, dynamic, sort_count)
            assert np.array_equal(lists[1], lists[2]), ("device", integer, dynamic, sort_count)
            if sort_count == n and indexes is None:                     # distances differ -> not the reversed identity
                assert not np.array_equal(lists[1], np.arange(n, dtype=np.uint32)[::-1])
    m.dispose()


def test_gathered_list_with_device_distances(ctx):
    n = 60_000
    centers = make_centers(n, seed=21)
    m = build_mesh(ctx, n, False, centers, np.zeros(n, np.uint32))
    tree = SplatTree(ctx)
    tree.process_splat_mesh(centers)
    cam = camera.demo_camera("garden", 640, 360)
    mvp = np.asarray(cam.sort_mvp(), np.float64).reshape(16)
    for integer in (True, False):
        w = SortWorker(ctx, n, integer, False)
        w.set_uploaded_count(n)
        g = tree.gather_scene_nodes_for_sort(cam, sort_worker=w)
        listed = np.asarray(g["indexesToSort"], np.uint32)[: g["splatRenderCount"]].copy()
        host = device_distances(m, mvp, integer, False, n)
        m.compute_distances_on_gpu(mvp, sort_worker=w, integer=integer, dynamic=False)
        for sort_count in (listed.size, listed.size // 4):
            got = w.sort_gathered(mvp, sort_count=sort_count, precomputed_on_device=True)["sortedIndexes"]
            c4 = js_integer_centers(centers) if integer else util.float_centers(centers)
            want = oracle.sort_indexes(listed, c4, mvp.astype(np.float32), sort_count=sort_count, render_count=listed.size,
                                       use_int=integer, precomputed=host)
            assert np.array_equal(got, want), (integer, sort_count)
            if sort_count == listed.size:
                g = tree.gather_scene_nodes_for_sort(cam, sort_worker=w)   # the partial sort below re-sorts the same list
        w.terminate()
    tree.dispose()
    m.dispose()


def test_errors(ctx):
    lib = ctx.lib
    n = 1000
    centers = make_centers(n, seed=2)
    m = SplatMesh(ctx, n, dynamic_mode=True)
    m.build(centers, np.zeros((n, 6), np.float32), np.zeros((n, 4), np.uint8))
    u = np.zeros(16 * 32, np.float32)
    call = lambda flags, scenes, dst=None: lib.gs_mesh_compute_distances(m.handle, flags, u.ctypes.data, scenes, None, dst)
    assert call(L.GS_SORT_INTEGER, 0) == L.GS_ERR_INVALID                       # scene_count 0
    assert call(L.GS_SORT_INTEGER, 33) == L.GS_ERR_INVALID                      # > GS_MAX_SCENES
    assert call(L.GS_SORT_DYNAMIC, 3) == L.GS_ERR_INVALID                       # several scenes, no scene indexes
    assert call(L.GS_SORT_DYNAMIC, 1) == L.GS_OK
    assert call(8, 1) == L.GS_ERR_INVALID                                       # unknown flag
    small = SortWorker(ctx, n - 1, True, False)
    assert call(L.GS_SORT_INTEGER, 1, small.handle) == L.GS_ERR_INVALID         # dst too small
    small.terminate()

    mvp = np.asarray(mvp_for(0), np.float32)
    w = SortWorker(ctx, n, True, False)
    w.set_uploaded_count(n)
    sort = lambda: lib.gs_sorter_sort(w.handle, mvp.ctypes.data, None, n, n, L.GS_PRECOMPUTED_DEVICE, None, None, None)
    assert sort() == L.GS_ERR_INVALID                                           # never received device distances
    m.compute_distances_on_gpu(mvp_for(0), sort_worker=w, integer=False, dynamic=False)
    assert sort() == L.GS_ERR_INVALID                                           # computed as float, sorter is integer
    m.compute_distances_on_gpu(mvp_for(0), sort_worker=w, integer=True, dynamic=False)
    assert sort() == L.GS_OK
    gath = lambda: lib.gs_sorter_sort_gathered(w.handle, mvp.ctypes.data, n, L.GS_PRECOMPUTED_DEVICE, None, None, None)
    big = SortWorker(ctx, 2 * n, True, False)
    big.set_uploaded_count(2 * n)                                               # more splats than the distances cover
    m.compute_distances_on_gpu(mvp_for(0), sort_worker=big, integer=True, dynamic=False)
    assert lib.gs_sorter_sort(big.handle, mvp.ctypes.data, None, n, n, L.GS_PRECOMPUTED_DEVICE, None, None, None) == L.GS_ERR_INVALID
    host = np.zeros(n, np.int32)                                                # a host sort overwrites the device distances
    assert lib.gs_sorter_sort(w.handle, mvp.ctypes.data, None, n, n, host.ctypes.data, None, None, None) == L.GS_OK
    assert sort() == L.GS_ERR_INVALID
    assert gath() == L.GS_ERR_INVALID                                           # (no gathered list either)
    big.terminate()
    w.terminate()
    m.dispose()
