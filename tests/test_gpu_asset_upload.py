"""-m gpu: the device decode of .ksplat / PLY assets (gs_mesh_upload_asset, gs_sorter_upload_asset_centers; csrc/asset_decode.hip)
against the host path it replaces (gs_asset_fill -> gs_mesh_upload [+ gs_mesh_upload_sh_u8] and util.integer_centers /
float_centers -> gs_sorter_upload_centers).  The host readers are pinned bit for bit to the reference's own loaders
(tests/test_assets_ref.py), so "device decode == host decode, bit for bit" pins the device path to the reference too.

Every case builds mesh + sorter A through the host path and mesh + sorter B through the new calls in one context and requires
np.array_equal - no tolerance - on: the sorted index list returned to the host, the frame rendered with it from a fixed camera
(scenes.CONFIGS' garden pose), gs_mesh_compute_distances' output (it reads the stored centres by original index) and the planes
gs_mesh_debug_read exposes per splat (records, rects, visibility mask of the draw).  The scene's centre sums are reduced in
another order on the device path; they feed scheduling heuristics only, so schedule words are not compared."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import asset_transform_cases
import ksplat_sections
from gaussiansplats3d_amd import Context, SplatMesh, assets, camera, create_sort_worker, scenes, util
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NODE_DIR = os.path.join(ROOT, "node")
W, H = 320, 180
CAM = camera.demo_camera(scenes.CONFIGS["C3"]["pose"], W, H)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the two paths
def host_upload(mesh, filled, frm, first, count):
    """gs_asset_fill's arrays [first, first + count) -> gs_mesh_upload (+ gs_mesh_upload_sh_u8) at [frm, frm + count)."""
    s = slice(first, first + count)
    p = lambda a: np.ascontiguousarray(a[s]) if a is not None else None      # noqa: E731
    c, cov, cov16, rgba, sh16, sh8 = (p(filled[k]) for k in ("centers", "cov", "cov_f16", "rgba", "sh_f16", "sh_u8"))
    d = lambda a: a.ctypes.data if a is not None else None                   # noqa: E731
    L.check(mesh.lib.gs_mesh_upload(mesh.handle, frm, count, d(c), d(cov), d(cov16), d(rgba), d(sh16)))
    if sh8 is not None:
        L.check(mesh.lib.gs_mesh_upload_sh_u8(mesh.handle, frm, count, d(sh8)))
    mesh.splat_count = max(mesh.splat_count, frm + count)


def host_centers(worker, filled, frm, first, count):
    c = filled["centers"][first:first + count]
    msg = util.integer_centers(c) if worker.integer_based_sort else util.float_centers(c)
    worker.post_message({"centers": msg, "range": {"from": frm, "to": frm + count - 1, "count": count}})


class Pair:
    """One mesh + one sorter sized for the asset, and what a sort + draw of them shows."""

    def __init__(self, ctx, asset, n, half, integer, keep_order, minimum_alpha, cam=CAM):
        info = asset.info
        self.asset, self.n, self.min_alpha, self.half, self.cam = asset, n, minimum_alpha, half, cam
        self.mesh = SplatMesh(ctx, n, info.sh_degree, half_precision_covariances=half,
                              spherical_harmonics_8bit=info.sh_level == 2 and info.sh_degree > 0, keep_order=keep_order)
        if self.mesh.sh_8bit:                                # the file's 8-bit SH range (a per-scene uniform)
            self.mesh.set_scenes(sh8_range=[(info.sh_min, info.sh_max)])
        self.worker = create_sort_worker(ctx, n, integer_based_sort=integer)
        self._filled = None

    @property
    def filled(self):
        if self._filled is None:
            with np.errstate(all="ignore"):
                self._filled = self.asset.fill(self.min_alpha, self.half)
        return self._filled

    def host(self, frm, first, count):
        host_upload(self.mesh, self.filled, frm, first, count)
        with np.errstate(all="ignore"):                   # hostile rows: NaN / infinite centres through integer_centers
            host_centers(self.worker, self.filled, frm, first, count)

    def device(self, frm, first, count):
        self.asset.upload_to(self.mesh, frm, first, count, self.min_alpha)
        self.asset.upload_centers_to(self.worker, frm, first, count)

    def observe(self):
        n = self.n
        reply = self.worker.post_message({"sort": {"modelViewProj": self.cam.sort_mvp(), "splatRenderCount": n, "splatSortCount": n}})
        order = reply["sortedIndexes"].copy()
        self.mesh.set_camera(self.cam)
        self.mesh.update_render_indexes(order, n)
        frame, _ = self.mesh.render()
        recs, rects, vis = self.mesh.debug_records(n)
        dist = np.empty(n, np.int32)
        self.mesh.compute_distances_on_gpu(self.cam.sort_mvp(), out=dist, integer=True)
        return {"order": order, "frame": frame, "records": recs, "rects": rects, "visible": vis, "distances": dist}

    def close(self):
        self.worker.terminate()
        self.mesh.dispose()


def assert_same(a, b, tag=""):
    for k in ("order", "distances", "visible", "rects", "records", "frame"):
        assert np.array_equal(a[k], b[k]), f"{tag}: {k} differs between the host path and the device decode"


def compare_whole(ctx, data, fmt, sh_degree, half, integer, keep_order, minimum_alpha, expect_pixels=True):
    asset = assets.SplatAsset(data, fmt, sh_degree)
    n = asset.info.splat_count
    a = Pair(ctx, asset, n, half, integer, keep_order, minimum_alpha)
    b = Pair(ctx, asset, n, half, integer, keep_order, minimum_alpha)
    try:
        a.host(0, 0, n)
        b.device(0, 0, n)
        oa, ob = a.observe(), b.observe()
        if expect_pixels:
            assert oa["frame"].any() and oa["visible"].any(), "the camera sees nothing: the case would compare empty frames"
        assert_same(oa, ob)
    finally:
        a.close()
        b.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ reference-written files
def _golden(case, tag):
    g = np.load(os.path.join(GOLDEN, f"assets_ref_{case}.npz"))
    man = json.loads(bytes(g["manifest"]).decode())
    if tag == "ply":
        return bytes(g["ply_bytes"]), "ply", man["shDegree"]
    return bytes(g[f"{tag}_ksplat"]), "ksplat", man["shDegree"]


@pytest.mark.parametrize("keep_order", [False, True])
@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("minimum_alpha", [1, 40])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("tag", ["ply", "gen0", "gen1", "gen2"])
@pytest.mark.parametrize("case", ["sh0", "sh1", "sh2"])
def test_reference_written_files(ctx, case, tag, half, minimum_alpha, integer, keep_order):
    """The PLY and the level 0 / 1 / 2 .ksplat the reference's own loaders wrote and read (tests/golden/assets_ref_*.npz)."""
    data, fmt, deg = _golden(case, tag)
    compare_whole(ctx, data, fmt, deg, half, integer, keep_order, minimum_alpha)


# ------------------------------------------------------------------------------------------------ larger synthetic files
def synthetic_splats(n, sh_degree, seed):
    rng = np.random.default_rng(seed)
    scene = scenes.scene_like(n, 0, scenes.SEED_BASE + seed)             # centres laid out for the garden pose
    scales = np.exp(rng.normal(-3.6, 0.5, size=(n, 3)))
    rot = rng.normal(size=(n, 4))
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    ncomp = {0: 0, 1: 9, 2: 24}[sh_degree]
    sh = rng.normal(0.0, 0.4, size=(n, ncomp)) if ncomp else None
    return scene.centers, scales, rot, rgba, sh


def ksplat_header(data):
    """What the parsed header says about the first section's buckets."""
    h = 4096
    bucket_size, bucket_count = struct.unpack_from("<II", data, h + 8)
    full, partial = struct.unpack_from("<II", data, h + 32)
    return {"level": struct.unpack_from("<H", data, 20)[0], "splats": struct.unpack_from("<I", data, h + 4)[0],
            "bucket_size": bucket_size, "buckets": bucket_count, "full": full, "partial": partial}


_SYNTH = {}


def synthetic_file(n, level, sh_degree, block_size=2.0, bucket_size=256, seed=5):
    key = (n, level, sh_degree, block_size, bucket_size, seed)
    if key not in _SYNTH:
        c, s, q, rgba, sh = synthetic_splats(n, sh_degree, seed)
        _SYNTH[key] = assets.write_ksplat(c, s, q, rgba, sh, sh_degree, level, block_size=block_size, bucket_size=bucket_size,
                                          sh_range=(-1.2, 1.3))[0]
    return _SYNTH[key]


@pytest.mark.parametrize("sh_degree", [0, 1, 2])
@pytest.mark.parametrize("level", [1, 2])
def test_larger_synthetic_files(ctx, level, sh_degree):
    """300 k seeded splats through assets.write_ksplat: many full buckets and partial ones, asserted from the header."""
    n = 300_000
    data = synthetic_file(n, level, sh_degree)
    hd = ksplat_header(data)
    assert hd["level"] == level and hd["splats"] == n
    assert hd["full"] >= 100 and hd["partial"] >= 2 and hd["buckets"] == hd["full"] + hd["partial"], hd   # both bucket paths are taken
    assert hd["full"] * hd["bucket_size"] < n, "no splat lies in a partial bucket"
    compare_whole(ctx, data, "ksplat", sh_degree, half=level == 2, integer=sh_degree != 1, keep_order=False, minimum_alpha=1)


# ------------------------------------------------------------------------------------------------ ranges
def ranges_case(ctx, plans, level=2, sh_degree=1, n=24_000):
    """plans: per pair, a list of (path, frm, first, count); every pair must end up showing the same as the first (all host)."""
    data = synthetic_file(n, level, sh_degree, block_size=4.0, bucket_size=128, seed=9)
    hd = ksplat_header(data)
    assert hd["full"] >= 8 and hd["partial"] >= 2
    asset = assets.SplatAsset(data, "ksplat", sh_degree)
    pairs = [Pair(ctx, asset, n, False, True, False, 1) for _ in plans]
    try:
        seen = []
        for pair, plan in zip(pairs, plans):
            for path, frm, first, count in plan:
                (pair.host if path == "host" else pair.device)(frm, first, count)
            seen.append(pair.observe())
        assert seen[0]["frame"].any()
        for k in range(1, len(seen)):
            assert_same(seen[0], seen[k], f"plan {k}")
    finally:
        for pair in pairs:
            pair.close()
        asset.close()


def test_progressive_load_in_three_unequal_pieces(ctx):
    n = 24_000
    cuts = [(0, 5_001), (5_001, 7_777), (12_778, n - 12_778)]
    ranges_case(ctx, [[("host", f, f, c) for f, c in cuts], [("device", f, f, c) for f, c in cuts]], n=n)


def test_first_differs_from_from(ctx):
    n = 24_000
    moves = [(100, 0, n - 100), (0, n - 100, 100)]                      # the file rotated by 100 splats
    ranges_case(ctx, [[("host", f, s, c) for f, s, c in moves], [("device", f, s, c) for f, s, c in moves]], n=n)


def test_reupload_of_an_overlapping_range(ctx):
    """[4000, 6000) is uploaded twice: the second call's non-fresh segment keeps its slots, [6000, n) is fresh."""
    n = 24_000
    moves = [(0, 0, 6_000), (4_000, 4_000, n - 4_000)]
    ranges_case(ctx, [[("host", f, s, c) for f, s, c in moves], [("device", f, s, c) for f, s, c in moves]], n=n)


def test_host_and_device_uploads_mix(ctx):
    n = 24_000
    k = 9_999
    ranges_case(ctx, [[("host", 0, 0, k), ("host", k, k, n - k)],
                      [("host", 0, 0, k), ("device", k, k, n - k)],
                      [("device", 0, 0, k), ("host", k, k, n - k)]], n=n)


# ------------------------------------------------------------------------------------------------ several sections
@pytest.mark.parametrize("transform", [None, "rigid"])
@pytest.mark.parametrize("degrees", [(1, 1), (1, 2)])
@pytest.mark.parametrize("level", [1, 2])
def test_several_sections(ctx, level, degrees, transform):
    """301 splats, an empty section, 310 splats (tests/ksplat_sections.py; with degrees (1, 2) the last section's rows are longer
    than the first's): the whole file, a range from inside the first section's partial buckets to inside the last section (the
    staged first section starts before the staged bytes, and the range crosses the empty section) and a range wholly in the
    last section, decoded on the device among host uploads of the rest, against the all-host pair."""
    data = ksplat_sections.three_sections(level, degrees)
    heads = ksplat_sections.section_headers(data)
    n_a, n_b = heads[0]["splats"], heads[2]["splats"]
    assert (n_a, heads[1]["splats"], n_b) == (301, 0, 310)
    for h in (heads[0], heads[2]):
        assert h["full"] >= 1 and h["partial"] >= 2 and h["full"] * h["bucket_size"] < h["splats"], h
    n = n_a + n_b
    crossing = (heads[0]["full"] * heads[0]["bucket_size"] + 5, n_a + n_b // 2)      # [begin, end)
    last = (n_a + 7, n - 13)
    assert heads[0]["full"] * heads[0]["bucket_size"] < crossing[0] < n_a < crossing[1] < n and n_a < last[0] < last[1] < n

    def around(begin, end):
        return [("host", 0, 0, begin), ("device", begin, begin, end - begin), ("host", end, end, n - end)]

    asset = assets.SplatAsset(data, "ksplat", 2)
    pairs = []
    try:
        assert asset.info.sh_degree == 1
        if transform:
            asset.set_transform(asset_transform_cases.matrix(transform))
        with np.errstate(all="ignore"):
            cam = asset_transform_cases.cloud_camera(asset.fill()["centers"])
        plans = [[("host", 0, 0, n)], [("device", 0, 0, n)], around(*crossing), around(*last)]
        seen = []
        for plan in plans:
            pair = Pair(ctx, asset, n, level == 2, transform is None, False, 1, cam=cam)
            pairs.append(pair)
            for path, frm, first, count in plan:
                (pair.host if path == "host" else pair.device)(frm, first, count)
            seen.append(pair.observe())
        assert seen[0]["frame"].any() and seen[0]["visible"].mean() >= 0.25, "the camera sees too little of the file"
        for k in range(1, len(seen)):
            assert_same(seen[0], seen[k], f"plan {k}")
    finally:
        for pair in pairs:
            pair.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ hostile rows
def _hostile_level0(n=6_000):
    c, s, q, rgba, sh = synthetic_splats(n, 1, 21)
    data = bytearray(assets.write_ksplat(c, s, q, rgba, sh, 1, 0)[0])
    bps, base = 44 + 4 * 9, 4096 + 1024
    row = lambda i: base + i * bps                                          # noqa: E731
    struct.pack_into("<f", data, row(10), float("nan"))                     # NaN centre x
    struct.pack_into("<f", data, row(11) + 4, float("inf"))                 # infinite centre y
    struct.pack_into("<f", data, row(12) + 8, float("-inf"))
    struct.pack_into("<ffff", data, row(13) + 24, 0.0, 0.0, 0.0, 0.0)       # zero quaternion
    struct.pack_into("<fff", data, row(14) + 12, 0.0, 0.0, 0.0)             # zero scale
    struct.pack_into("<f", data, row(15) + 12, float("nan"))                # NaN scale
    struct.pack_into("<f", data, row(16) + 44, float("inf"))                # infinite SH coefficient
    for i in range(17, 40):
        data[row(i) + 43] = 0                                               # alpha 0
    struct.pack_into("<fff", data, row(41), 3e9, -3e9, 1e-30)               # x1000 leaves int32
    return bytes(data)


def _hostile_level1(n=6_000):
    c, s, q, rgba, sh = synthetic_splats(n, 1, 22)
    data = bytearray(assets.write_ksplat(c, s, q, rgba, sh, 1, 1, block_size=4.0, bucket_size=64)[0])
    hd = ksplat_header(data)
    assert hd["full"] >= 2 and hd["partial"] >= 2
    buckets = 4096 + 1024 + 4 * hd["partial"]
    rows = buckets + 12 * hd["buckets"]
    bps = 24 + 2 * 9
    struct.pack_into("<f", data, buckets + 12 * 0, float("nan"))            # a full bucket's centre: 64 NaN centres
    struct.pack_into("<f", data, buckets + 12 * 1 + 4, float("inf"))
    struct.pack_into("<f", data, buckets + 12 * (hd["buckets"] - 1) + 8, float("-inf"))   # the last partial bucket
    struct.pack_into("<HHHH", data, rows + 200 * bps + 12, 0, 0, 0, 0)      # zero quaternion (half bits)
    struct.pack_into("<HHH", data, rows + 201 * bps + 6, 0, 0, 0)           # zero scale
    struct.pack_into("<H", data, rows + 202 * bps + 6, 0x7E00)              # NaN scale
    struct.pack_into("<H", data, rows + 203 * bps + 12, 0x7C00)             # infinite rotation component
    for i in range(204, 230):
        data[rows + i * bps + 23] = 0                                       # alpha 0
    return bytes(data)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("maker", [_hostile_level0, _hostile_level1])
def test_hostile_rows(ctx, maker, half, integer):
    """NaN and infinite centres, a zero quaternion, zero / NaN scales and alpha 0 rows: same planes and frames as the host path."""
    data = maker()
    a = assets.SplatAsset(data, "ksplat", 1)
    with np.errstate(all="ignore"):
        c = a.fill()["centers"]
    a.close()
    assert np.isnan(c).any() and np.isinf(c).any(), "the hostile centres did not reach the decoded arrays"
    compare_whole(ctx, data, "ksplat", 1, half, integer, keep_order=False, minimum_alpha=1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(ctx):
    n = 24_000
    data2 = synthetic_file(n, 2, 1, block_size=4.0, bucket_size=128, seed=9)       # level 2: uint8 SH
    data1 = synthetic_file(n, 1, 1, block_size=4.0, bucket_size=128, seed=9)       # level 1: half SH
    asset2, asset1 = assets.SplatAsset(data2, "ksplat", 1), assets.SplatAsset(data1, "ksplat", 1)
    asset_deg0 = assets.SplatAsset(data1, "ksplat", 0)
    pair = Pair(ctx, asset1, n, False, True, False, 1)                              # a half-SH mesh of degree 1
    try:
        pair.device(0, 0, n)
        before = pair.observe()
        assert before["frame"].any()

        def refused(call):
            with pytest.raises(L.GsError) as e:
                call()
            assert e.value.status == L.GS_ERR_INVALID

        refused(lambda: asset_deg0.upload_to(pair.mesh, 0, 0, n))                   # SH degree 0 file into a degree 1 mesh
        refused(lambda: asset2.upload_to(pair.mesh, 0, 0, n))                       # uint8 SH into a mesh without GS_MESH_SH_U8
        refused(lambda: asset1.upload_to(pair.mesh, 0, n - 10, 11))                 # first + count leaves the asset
        refused(lambda: asset1.upload_to(pair.mesh, n - 10, 0, 11))                 # from + count leaves the mesh
        refused(lambda: asset1.upload_centers_to(pair.worker, 0, n - 10, 11))
        refused(lambda: asset1.upload_centers_to(pair.worker, n - 10, 0, 11))
        mesh8 = SplatMesh(ctx, n, 1, spherical_harmonics_8bit=True)
        refused(lambda: asset1.upload_to(mesh8, 0, 0, n))                           # half SH into a GS_MESH_SH_U8 mesh
        mesh8.dispose()
        assert_same(before, pair.observe(), "after the refused calls")
    finally:
        pair.close()
        for a in (asset1, asset2, asset_deg0):
            a.close()


# ------------------------------------------------------------------------------------------------ Node
def test_mesh_upload_asset_through_node_matches_the_python_mirror(ctx, tmp_path):
    """meshUploadAsset + a draw through node/gsplat.js equals the Python mirror's frame of the same file."""
    assert shutil.which("node") is not None, "node is not installed"
    subprocess.check_call(["make", "-C", NODE_DIR], stdout=subprocess.DEVNULL)
    n = 24_000
    data = synthetic_file(n, 2, 1, block_size=4.0, bucket_size=128, seed=9)
    asset = assets.SplatAsset(data, "ksplat", 1)
    pair = Pair(ctx, asset, n, False, True, False, 1)
    try:
        pair.device(0, 0, n)
        seen = pair.observe()
    finally:
        pair.close()
        asset.close()
    fpath, ipath, opath = str(tmp_path / "a.ksplat"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fpath, "wb").write(data)
    fx, fy = CAM.focal()
    with open(ipath, "wb") as f:
        for p in (np.array([W, H, 1, 1], np.uint32), np.asarray(CAM.model_view(), np.float64).astype(np.float32),
                  np.asarray(CAM.projection, np.float64).astype(np.float32), np.asarray(CAM.position, np.float32),
                  np.array([fx, fy], np.float32), np.asarray(CAM.sort_mvp(), np.float64).astype(np.float32)):
            f.write(np.ascontiguousarray(p).tobytes())
    res = subprocess.run(["node", "asset_upload_via_js.js", fpath, ipath, opath], cwd=NODE_DIR, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["splatCount"] == n
    raw = np.fromfile(opath, dtype=np.uint8)
    order = raw[:4 * n].view(np.uint32)
    frame = raw[4 * n:].reshape(H, W, 4)
    assert np.array_equal(order, seen["order"]), "sorterUploadAssetCenters + sort differs from the Python mirror"
    assert frame.any() and np.array_equal(frame, seen["frame"]), "meshUploadAsset + draw differs from the Python mirror"
