"""-m gpu: the device .ksplat encoder (gs_asset_encode_ksplat, csrc/asset_encode.hip) against the reference's writer.

Every case of tests/golden/ksplat_encode_ref.npz (what SplatBuffer.generateFromUncompressedSplatArrays returned under Node) must
come back byte for byte, with the order the host model of tests/test_ksplat_encode_ref.py gives; everything the golden cannot
hold - the other five formats' row sources, sizes at the kernels' own boundaries, a scene of 70 000 splats - is held to that
model, which the CPU tier pins to the golden.  The model's input for a format whose rows the asset keeps as a file is the
level-0 image the host readers lay those rows out as (pinned to the reference's parsers by the tests of each format)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_asset_upload as U
import test_ksplat_encode_ref as R
from gaussiansplats3d_amd import Context, assets
from gaussiansplats3d_amd import _lib as L
from oracle import asset_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def level0_image(asset):
    """The asset's level-0 rows as a one-section image (the library's debug entry; copied)."""
    lib = asset.lib
    lib.gs_debug_asset_level0_image.restype = C.c_int
    lib.gs_debug_asset_level0_image.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    data, size = C.c_void_p(), C.c_uint64()
    L.check(lib.gs_debug_asset_level0_image(asset.handle, C.byref(data), C.byref(size)))
    return C.string_at(data, size.value)


def encode(ctx, asset, **kw):
    out, order = asset.encode_ksplat(ctx, **kw)
    try:
        return out.to_bytes(), order, (out.info.splat_count, out.info.sh_degree, out.info.compression_level)
    finally:
        out.close()


def against_model(ctx, data, fmt, degree, level, minimum_alpha=1, block_size=5.0, bucket_size=256, scene_center=(0.0, 0.0, 0.0)):
    asset = assets.SplatAsset(data, fmt, degree)
    try:
        rows = R.level0_rows(level0_image(asset))
        assert rows["degree"] == asset.info.sh_degree
        want = R.model_encode(rows, level, minimum_alpha, block_size, bucket_size, scene_center)
        got, order, info = encode(ctx, asset, compression_level=level, minimum_alpha=minimum_alpha, block_size=block_size,
                                  bucket_size=bucket_size, scene_center=scene_center)
    finally:
        asset.close()
    assert R.first_difference(got, want["bytes"]) is None
    assert np.array_equal(order, want["order"])
    assert info == (want["order"].size, rows["degree"], level)
    return want


# ------------------------------------------------------------------------------------------------ the reference's own output
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_golden_cases(ctx, case):
    want = R._Z[case["name"] + "_ksplat"].tobytes()
    asset = assets.SplatAsset(R._Z[case["input"] + "_file"].tobytes(), "ksplat", 2)
    try:
        out, order = asset.encode_ksplat(ctx, compression_level=case["compressionLevel"], minimum_alpha=case["minimumAlpha"],
                                         block_size=case["blockSize"], bucket_size=case["bucketSize"], scene_center=case["sceneCenter"])
    finally:
        asset.close()
    try:
        assert R.first_difference(out.to_bytes(), want) is None
        assert np.array_equal(order, R.model_of(case)["order"])
        with np.errstate(all="ignore"):
            got, exp = out.fill(minimum_alpha=1), asset_oracle.fill_from_ksplat(want, min_alpha=1)
    finally:
        out.close()
    assert (out.info.compression_level, exp["level"]) == (case["compressionLevel"],) * 2
    assert np.array_equal(got["centers"], exp["centers"], equal_nan=True) and np.array_equal(got["cov"], exp["cov"], equal_nan=True)
    assert np.array_equal(got["rgba"], exp["rgba"])
    if exp["sh_degree"]:
        assert np.array_equal(got["sh_u8"] if case["compressionLevel"] == 2 else got["sh_f16"], exp["sh"])


# ------------------------------------------------------------------------------------------------ the other row sources
FORMAT_N = 2_000
_SCENES = {}


def scene_file(kind):
    """(bytes, fmt, degree the file is read at): one seeded scene through the package's writers, at the degree the format holds."""
    if kind not in _SCENES:
        degree = {"ply_v1": 2, "splat": 0, "spz": 2, "compressed": 2, "inria_v2": 1}[kind]
        c, s, q, rgba, sh = U.synthetic_splats(FORMAT_N, degree, 61)
        unit, logit = rgba / 255.0, np.log((rgba[:, 3] + 0.5) / (255.5 - rgba[:, 3]))
        f_dc = (unit[:, :3] - 0.5) / 0.28209479177387814
        if kind == "ply_v1":
            _SCENES[kind] = (assets.write_ply(c, np.log(s), q, f_dc, logit, sh), "ply", degree)
        elif kind == "splat":
            _SCENES[kind] = (assets.write_splat(c, s, q, rgba), "splat", degree)
        elif kind == "spz":
            _SCENES[kind] = (assets.write_spz(c, np.log(s), q, unit, sh), "spz", degree)
        elif kind == "compressed":
            _SCENES[kind] = (assets.write_compressed_ply(c, np.log(s), q, unit, sh), "ply", degree)
        else:
            _SCENES[kind] = (assets.write_inria_v2_ply(c, np.log(s), q, f_dc, logit, sh), "ply", degree)
    return _SCENES[kind]


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("kind", ["ply_v1", "splat", "spz", "compressed", "inria_v2"])
def test_other_formats(ctx, kind, level):
    data, fmt, degree = scene_file(kind)
    want = against_model(ctx, data, fmt, degree, level, minimum_alpha=40, block_size=4.0, bucket_size=16)
    assert 0 < want["order"].size < FORMAT_N and want["full"] >= 2 and want["partial"] >= 2


def test_a_file_read_below_its_degree(ctx):
    data, fmt, _ = scene_file("compressed")
    against_model(ctx, data, fmt, 1, 2, block_size=4.0, bucket_size=16)


# ------------------------------------------------------------------------------------------------ sizes at the kernels' boundaries
def level0_file(n, degree, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    ncomp = R.NCOMP[degree]
    c = rng.normal(0.0, spread, size=(n, 3)).astype(np.float32)
    sh = rng.normal(0.0, 0.4, size=(n, ncomp)).astype(np.float32) if ncomp else None
    rgba = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
    return assets.write_ksplat(c, np.exp(rng.normal(-3.0, 0.5, size=(n, 3))).astype(np.float32), rng.normal(size=(n, 4)), rgba, sh, degree, 0)[0]


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3 * 4096 + 17])
def test_sizes(ctx, n, level):
    """One splat; a wave, a workgroup, a radix tile - each one short, exact and one over; rows of 80, 42 and 33 bytes, so the last
    workgroup's rows end at every byte phase of a dword.  minimum_alpha 0 keeps every row."""
    against_model(ctx, level0_file(n, 1, 100 + n), "ksplat", 1, level, minimum_alpha=0, block_size=2.0, bucket_size=16)


def test_sizes_with_dropped_rows(ctx):
    want = against_model(ctx, level0_file(3 * 4096 + 17, 2, 77), "ksplat", 2, 2, minimum_alpha=128, block_size=2.0, bucket_size=64)
    assert 4096 < want["order"].size < 2 * 4096 + 2048


def test_seventy_thousand_splats(ctx):
    want = against_model(ctx, level0_file(70_001, 0, 78, spread=4.0), "ksplat", 0, 1, minimum_alpha=1, block_size=4.0, bucket_size=256)
    assert want["full"] >= 100 and 200 <= want["partial"] <= 900


# ------------------------------------------------------------------------------------------------ refusals
def refused(ctx, asset, status, **kw):
    with pytest.raises(L.GsError) as e:
        asset.encode_ksplat(ctx, **kw)
    assert e.value.status == status, str(e.value)


def patched(data, row, column, value):
    out = bytearray(data)
    out[5120 + 44 * row + 4 * column:5120 + 44 * row + 4 * column + 4] = np.float32(value).tobytes()
    return bytes(out)


def test_refusals(ctx):
    data = level0_file(500, 0, 90)
    asset = assets.SplatAsset(data, "ksplat", 2)
    try:
        refused(ctx, asset, L.GS_ERR_INVALID, compression_level=3)
        for block in (-2.0, float("inf"), float("nan")):
            refused(ctx, asset, L.GS_ERR_INVALID, block_size=block)
        refused(ctx, asset, L.GS_ERR_INVALID, bucket_size=65536)
        refused(ctx, asset, L.GS_ERR_INVALID, minimum_alpha=256)                     # no splat survives
        refused(ctx, asset, L.GS_ERR_UNSUPPORTED, block_size=1e-3)                   # tens of thousands of blocks along every axis
        asset.set_transform(np.eye(4))
        refused(ctx, asset, L.GS_ERR_INVALID)
        asset.set_transform(None)
        got, _, _ = encode(ctx, asset)                                               # and the asset still encodes
        assert got == R.model_encode(R.level0_rows(data), 1)["bytes"]
        with pytest.raises(L.GsError) as e:
            asset.to_bytes()                                                         # a source is no encoder result
        assert e.value.status == L.GS_ERR_INVALID
    finally:
        asset.close()
    for level in (1, 2):
        quantised = assets.SplatAsset(R.model_encode(R.level0_rows(data), level)["bytes"], "ksplat", 2)
        try:
            refused(ctx, quantised, L.GS_ERR_UNSUPPORTED)
        finally:
            quantised.close()
    for value in (float("nan"), float("inf"), float("-inf")):
        broken = assets.SplatAsset(patched(data, 123, 1, value), "ksplat", 2)
        try:
            refused(ctx, broken, L.GS_ERR_INVALID)
            alpha = R.level0_rows(data)["rgba"][123, 3]
            if alpha < 255:                                                          # dropped, the row's centre is never looked at
                got, _, _ = encode(ctx, broken, minimum_alpha=int(alpha) + 1)
                assert got == R.model_encode(R.level0_rows(patched(data, 123, 1, value)), 1, int(alpha) + 1)["bytes"]
        finally:
            broken.close()


# ------------------------------------------------------------------------------------------------ what the encoder must not depend on
def test_poisoned_allocations_change_no_byte(monkeypatch):
    """Under GSPLAT_POISON_ALLOC=0xFF every fresh allocation holds 0xFF: a flag, count or table word read before it was written shows."""
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", "0xFF")                                # (read at every allocation: stays set for the whole test)
    pctx = Context(0)
    try:
        for name in ("sh2_l2", "exact_l1", "single_l1", "dropped_l2", "nonneg_l2"):
            case = next(c for c in R.CASES if c["name"] == name)
            asset = assets.SplatAsset(R._Z[case["input"] + "_file"].tobytes(), "ksplat", 2)
            try:
                got, _, _ = encode(pctx, asset, compression_level=case["compressionLevel"], minimum_alpha=case["minimumAlpha"],
                                   block_size=case["blockSize"], bucket_size=case["bucketSize"], scene_center=case["sceneCenter"])
            finally:
                asset.close()
            assert R.first_difference(got, R._Z[name + "_ksplat"].tobytes()) is None, name
        against_model(pctx, level0_file(3 * 4096 + 17, 1, 79), "ksplat", 1, 2, minimum_alpha=100, block_size=2.0, bucket_size=16)
    finally:
        pctx.close()


def test_a_meshs_next_frame_is_unchanged(ctx):
    """No kernel of a draw or a sort takes part in an encode, and none of their buffers: the frame after it is the frame before it."""
    data = U.synthetic_file(24_000, 0, 1)
    asset = assets.SplatAsset(data, "ksplat", 2)
    pair = U.Pair(ctx, asset, 24_000, False, True, False, 1)
    try:
        pair.device(0, 0, 24_000)
        before = pair.observe()
        assert before["frame"].any()
        encode(ctx, asset, compression_level=2, block_size=2.0)
        U.assert_same(before, pair.observe(), "after an encode")
    finally:
        pair.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ Node
def test_encode_through_node_equals_the_python_bytes(ctx, tmp_path):
    """node/asset_encode_via_js.js: encodeKsplat(asset, options) returns the Buffer the Python mirror returns."""
    assert shutil.which("node") is not None, "node is not installed"
    subprocess.check_call(["make", "-C", U.NODE_DIR], stdout=subprocess.DEVNULL)
    data, fmt, degree = scene_file("compressed")
    asset = assets.SplatAsset(data, fmt, degree)
    try:
        want, _, _ = encode(ctx, asset, compression_level=2, minimum_alpha=40, block_size=4.0, bucket_size=16, scene_center=(0.5, 0.25, -1.0))
    finally:
        asset.close()
    fpath, opath = str(tmp_path / "scene.ply"), str(tmp_path / "scene.ksplat")
    open(fpath, "wb").write(data)
    res = subprocess.run(["node", "asset_encode_via_js.js", fpath, opath, "2", "40", "0.5,0.25,-1", "4", "16", str(degree)], cwd=U.NODE_DIR,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    got = open(opath, "rb").read()
    assert info["bytes"] == len(got) and R.first_difference(got, want) is None
