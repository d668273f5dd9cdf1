"""-m gpu: the device decode of .splat and PlayCanvas compressed PLY assets (the row sources of csrc/asset_decode.hip) against
the host path (gs_asset_fill over the level-0 image the host builds from the same rows -> gs_mesh_upload, util centres ->
gs_sorter_upload_centers).  Both sides call one row arithmetic (csrc/asset_internal.hpp, its own exp included), and the host
readers are pinned bit for bit to the reference's parsers (tests/test_assets_formats_ref.py), so the comparison is
np.array_equal - no tolerance - on what tests/test_gpu_asset_upload.py compares: the sorted index list of an integer and a
float sorter, distances, the debug planes and one small frame.  That file's helpers are imported, not restated."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import asset_formats_cases as FC
import test_gpu_asset_upload as U
from gaussiansplats3d_amd import Context, SplatMesh, assets
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
N = 24_000                                   # 93 full chunks and one of 192 splats
KINDS = ["splat", "pc_sh0", "pc_sh1", "pc_sh2", "pc_sh3"]
NCOEF = {"pc_sh0": 0, "pc_sh1": 9, "pc_sh2": 24, "pc_sh3": 45}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_FILES = {}


def synthetic_file(kind, n=N, seed=31):
    """(bytes, fmt, output SH degree): seeded splats laid out for the shared camera, through the package's writers."""
    key = (kind, n, seed)
    if key not in _FILES:
        ncoef = NCOEF.get(kind, 0)
        c, s, q, rgba, _ = U.synthetic_splats(n, 0, seed)
        rng = np.random.default_rng(seed + 1)
        if kind == "splat":
            _FILES[key] = (assets.write_splat(c, s, q, rgba), "splat", 0)
        else:
            sh = rng.normal(0.0, 0.4, size=(n, ncoef)) if ncoef else None
            data = assets.write_compressed_ply(c, np.log(s), q, rgba / 255.0, sh, color_extremes=kind in ("pc_sh1", "pc_sh3"))
            _FILES[key] = (data, "ply", min(2, {0: 0, 9: 1, 24: 2, 45: 3}[ncoef]))
    return _FILES[key]


# ------------------------------------------------------------------------------------------------ reference-checked files
@pytest.mark.parametrize("minimum_alpha", [1, 40])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", FC.cases())
def test_golden_cases(ctx, name, half, minimum_alpha):
    """Every file of tests/golden/assets_formats_ref.npz (NaN rotations, colour lerps on .5, alpha 0 / 39 / 40 included)."""
    data, fmt, degree, _ = FC.case(name)
    U.compare_whole(ctx, data, fmt, degree, half, integer=not half, keep_order=False, minimum_alpha=minimum_alpha)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_whole_synthetic_file(ctx, kind, integer):
    data, fmt, degree = synthetic_file(kind)
    a = assets.SplatAsset(data, fmt, 2)
    assert (a.info.splat_count, a.info.sh_degree) == (N, degree)
    a.close()
    U.compare_whole(ctx, data, fmt, 2, half=kind == "pc_sh2", integer=integer, keep_order=False, minimum_alpha=1)


@pytest.mark.parametrize("kind", ["splat", "pc_sh1"])
def test_257_splats(ctx, kind):
    """One full workgroup / chunk and one splat."""
    data, fmt, _ = synthetic_file(kind, n=257)
    U.compare_whole(ctx, data, fmt, 2, False, True, False, 1)


# ------------------------------------------------------------------------------------------------ ranges
def cuts(points):
    return [(a, a, b - a) for a, b in zip(points[:-1], points[1:])]


LAST_CHUNK = N // 256 * 256                  # 23 808: the partial chunk of 192 splats
PLANS = {
    # first = 300, count = 1000 starts inside chunk 1 and spans five; one splat at 7000; the last partial chunk alone
    "inside_chunks": cuts([0, 300, 1300, 7000, 7001, LAST_CHUNK, N]),
    # first = 511, count = 2 straddles two chunks; then three unequal progressive pieces
    "straddle_and_pieces": cuts([0, 511, 513, 5001, 12778, N]),
    "first_differs_from_from": [(100, 0, N - 100), (0, N - 100, 100)],            # the file rotated by 100 splats
    "overlapping_reupload": [(0, 0, 6000), (4000, 4000, N - 4000)],
}


def run_plans(ctx, kind, plans):
    """plans: per pair a list of (path, frm, first, count); every pair must show what the first (all host) shows."""
    data, fmt, degree = synthetic_file(kind)
    asset = assets.SplatAsset(data, fmt, 2)
    pairs = [U.Pair(ctx, asset, N, False, True, False, 1) for _ in plans]
    try:
        seen = []
        for pair, plan in zip(pairs, plans):
            for path, frm, first, count in plan:
                (pair.host if path == "host" else pair.device)(frm, first, count)
            seen.append(pair.observe())
        assert seen[0]["frame"].any() and seen[0]["visible"].any()
        for k in range(1, len(seen)):
            U.assert_same(seen[0], seen[k], f"{kind} plan {k}")
    finally:
        for pair in pairs:
            pair.close()
        asset.close()


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_ranges(ctx, kind, plan):
    moves = PLANS[plan]
    run_plans(ctx, kind, [[("host", f, s, c) for f, s, c in moves], [("device", f, s, c) for f, s, c in moves]])


@pytest.mark.parametrize("kind", KINDS)
def test_host_and_device_uploads_mix(ctx, kind):
    k = 9_999
    run_plans(ctx, kind, [[("host", 0, 0, k), ("host", k, k, N - k)], [("host", 0, 0, k), ("device", k, k, N - k)],
                          [("device", 0, 0, k), ("host", k, k, N - k)]])


# ------------------------------------------------------------------------------------------------ a scene transform
@pytest.mark.parametrize("kind", ["splat", "pc_sh2"])
def test_transformed(ctx, kind):
    """A non-uniform scale, a small rotation and a translation baked on both paths (the scene stays in front of the camera)."""
    data, fmt, _ = synthetic_file(kind)
    ang = 0.05
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    m = np.eye(4)
    m[:3, :3] = rot @ np.diag([1.1, 0.9, 1.05])
    m[:3, 3] = [0.1, -0.05, 0.02]
    asset = assets.SplatAsset(data, fmt, 2)
    asset.set_transform(m.T.reshape(-1))                     # column-major elements
    a, b = (U.Pair(ctx, asset, N, False, integer, False, 1) for integer in (True, True))
    try:
        a.host(0, 0, N)
        b.device(0, 0, N)
        oa, ob = a.observe(), b.observe()
        assert oa["frame"].any() and oa["visible"].any()
        U.assert_same(oa, ob, kind)
        plain = assets.SplatAsset(data, fmt, 2)
        assert not np.array_equal(plain.fill()["centers"], a.filled["centers"]), "the transform moved nothing"
        plain.close()
    finally:
        a.close()
        b.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ hostile rows
def _hostile_compressed(n=6_000):
    c, s, q, rgba, _ = U.synthetic_splats(n, 0, 23)
    rng = np.random.default_rng(24)
    sh = rng.normal(0.0, 0.4, size=(n, 9))
    words = {int(i): int(w) for i, w in zip(rng.choice(n, 300, replace=False), rng.integers(0, 1 << 32, 300, dtype=np.uint64))}
    data = bytearray(assets.write_compressed_ply(c, np.log(s), q, rgba / 255.0, sh, rotation_words=words))
    end = data.index(b"end_header\n") + 11
    ext = lambda chunk, k: end + 48 * chunk + 4 * k          # noqa: E731  min_x/y/z 0..2, max_x/y/z 3..5, min_scale 6..8, max_scale 9..11
    struct.pack_into("<f", data, ext(0, 0), float("nan"))                   # 256 NaN x
    struct.pack_into("<f", data, ext(1, 4), float("inf"))                   # max_y = +inf: inf, or inf * 0 = NaN at t = 0
    struct.pack_into("<f", data, ext(2, 2), float("-inf"))
    lo, hi = struct.unpack_from("<f", data, ext(3, 0))[0], struct.unpack_from("<f", data, ext(3, 3))[0]
    struct.pack_into("<f", data, ext(3, 0), hi)                             # min_x > max_x
    struct.pack_into("<f", data, ext(3, 3), lo)
    struct.pack_into("<f", data, ext(4, 9), 800.0)                          # exp overflows: infinite scales
    struct.pack_into("<f", data, ext(5, 6), -800.0)                         # exp underflows: zero and subnormal scales
    struct.pack_into("<f", data, ext(6, 10), float("nan"))                  # NaN scale extreme: `|| 0`
    struct.pack_into("<ff", data, ext(7, 7), 86.0, 89.5)                    # scales around fp32's overflow at exp(88.72)
    return bytes(data), "ply"


def _hostile_splat(n=6_000):
    c, s, q, rgba, _ = U.synthetic_splats(n, 0, 25)
    data = bytearray(assets.write_splat(c, s, q, rgba))
    struct.pack_into("<f", data, 32 * 10, float("nan"))
    struct.pack_into("<f", data, 32 * 11 + 4, float("inf"))
    struct.pack_into("<f", data, 32 * 12 + 8, float("-inf"))
    struct.pack_into("<f", data, 32 * 13 + 12, float("nan"))                # NaN scale
    struct.pack_into("<f", data, 32 * 14 + 16, float("inf"))                # infinite scale
    struct.pack_into("<fff", data, 32 * 15 + 12, 0.0, 0.0, 0.0)
    data[32 * 16 + 28:32 * 16 + 32] = bytes([128, 128, 128, 128])           # length-0 quaternion
    data[32 * 17 + 28:32 * 17 + 32] = bytes([0, 255, 0, 255])
    for i in range(18, 40):
        data[32 * i + 27] = 0                                               # alpha 0
    struct.pack_into("<fff", data, 32 * 41, 3e9, -3e9, 1e-30)               # x1000 leaves int32
    return bytes(data), "splat"


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("maker", [_hostile_compressed, _hostile_splat])
def test_hostile_rows(ctx, maker, half, integer):
    data, fmt = maker()
    a = assets.SplatAsset(data, fmt, 1)
    with np.errstate(all="ignore"):
        f = a.fill(1, False, want_scale_rotation=True)
    a.close()
    assert np.isnan(f["centers"]).any() and np.isinf(f["centers"]).any(), "the hostile centres did not reach the decoded arrays"
    assert np.isinf(f["scales"]).any() and (f["scales"] == 0).any()
    U.compare_whole(ctx, data, fmt, 1, half, integer, keep_order=False, minimum_alpha=1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(ctx):
    data1, fmt, _ = synthetic_file("pc_sh1")
    asset1, asset_deg0 = assets.SplatAsset(data1, fmt, 1), assets.SplatAsset(data1, fmt, 0)
    splat = assets.SplatAsset(synthetic_file("splat")[0], "splat")
    pair = U.Pair(ctx, asset1, N, False, True, False, 1)                            # a half-SH mesh of degree 1
    try:
        pair.device(0, 0, N)
        before = pair.observe()
        assert before["frame"].any()

        def refused(call):
            with pytest.raises(L.GsError) as e:
                call()
            assert e.value.status == L.GS_ERR_INVALID

        refused(lambda: asset_deg0.upload_to(pair.mesh, 0, 0, N))                   # SH degree 0 file into a degree 1 mesh
        refused(lambda: splat.upload_to(pair.mesh, 0, 0, N))
        refused(lambda: asset1.upload_to(pair.mesh, 0, N - 10, 11))                 # first + count leaves the asset
        refused(lambda: asset1.upload_to(pair.mesh, N - 10, 0, 11))                 # from + count leaves the mesh
        refused(lambda: asset1.upload_centers_to(pair.worker, 0, N - 10, 11))
        refused(lambda: splat.upload_centers_to(pair.worker, N - 10, 0, 11))
        mesh8 = SplatMesh(ctx, N, 1, spherical_harmonics_8bit=True)
        refused(lambda: asset1.upload_to(mesh8, 0, 0, N))                           # half SH (sh_level 1) into a GS_MESH_SH_U8 mesh
        mesh8.dispose()
        U.assert_same(before, pair.observe(), "after the refused calls")
    finally:
        pair.close()
        for a in (asset1, asset_deg0, splat):
            a.close()


# ------------------------------------------------------------------------------------------------ Node
@pytest.mark.parametrize("kind", ["splat", "pc_sh1"])
def test_round_trip_through_node(ctx, tmp_path, kind):
    """node/asset_formats_via_js.js (format from the extension / the header) draws what the Python mirror draws."""
    assert shutil.which("node") is not None, "node is not installed"
    subprocess.check_call(["make", "-C", U.NODE_DIR], stdout=subprocess.DEVNULL)
    data, fmt, degree = synthetic_file(kind)
    asset = assets.SplatAsset(data, fmt, 2)
    pair = U.Pair(ctx, asset, N, False, True, False, 1)
    try:
        pair.device(0, 0, N)
        seen = pair.observe()
    finally:
        pair.close()
        asset.close()
    fpath, ipath, opath = str(tmp_path / ("a.splat" if fmt == "splat" else "a.ply")), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fpath, "wb").write(data)
    cam = U.CAM
    fx, fy = cam.focal()
    with open(ipath, "wb") as f:
        for p in (np.array([U.W, U.H, degree, 0], np.uint32), np.asarray(cam.model_view(), np.float64).astype(np.float32),
                  np.asarray(cam.projection, np.float64).astype(np.float32), np.asarray(cam.position, np.float32),
                  np.array([fx, fy], np.float32), np.asarray(cam.sort_mvp(), np.float64).astype(np.float32)):
            f.write(np.ascontiguousarray(p).tobytes())
    res = subprocess.run(["node", "asset_formats_via_js.js", fpath, ipath, opath], cwd=U.NODE_DIR, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["splatCount"] == N and info["format"] == (3 if fmt == "splat" else 1)
    raw = np.fromfile(opath, dtype=np.uint8)
    assert np.array_equal(raw[:4 * N].view(np.uint32), seen["order"]), "sorterUploadAssetCenters + sort differs from the Python mirror"
    frame = raw[4 * N:].reshape(U.H, U.W, 4)
    assert frame.any() and np.array_equal(frame, seen["frame"]), "meshUploadAsset + draw differs from the Python mirror"
