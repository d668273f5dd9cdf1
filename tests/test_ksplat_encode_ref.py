"""CPU tier of the .ksplat encoder (gs_asset_encode_ksplat, csrc/asset_encode.hip).

The numpy model below is the reference's writer, SplatBuffer.generateFromUncompressedSplatArrays
(/root/reference/src/loaders/SplatBuffer.js:1050-1399), for one array of level-0 rows in file order: assets.write_ksplat's
data-parallel form of the bucket bookkeeping, with bucket order at level 0 too and the SH range rule as the plain sequential
loop it is.  It is held, byte for byte, to tests/golden/ksplat_encode_ref.npz (what the reference's writer returned under Node
for seeded level-0 rows: tests/tools/make_ksplat_encode_golden.py) and to the three files the reference wrote from the PLY
of tests/golden/assets_ref_sh*.npz; five mutations of it must each fail some golden case.  The GPU tier
(tests/test_gpu_ksplat_encode.py) holds the device encoder to this model.  Here, without a device: the refusals that need
none, the exported / declared / typed symbols, and the host-only layout function against the model's sizes and offsets."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest

import gaussiansplats3d_amd as g
from gaussiansplats3d_amd import _lib, assets
from gaussiansplats3d_amd.util import to_half_three

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NCOMP = {0: 0, 1: 9, 2: 24}
MUTATIONS = ("open_in_insertion_order", "centre_from_id", "true_sh_minimum", "no_reorder_at_level0", "rint_for_round")


# ------------------------------------------------------------------------------------------------ the model
def level0_rows(data):
    """The rows of a one-section level-0 .ksplat image: what an UncompressedSplatArray entry holds of each."""
    data = bytes(data)
    assert struct.unpack_from("<H", data, 20)[0] == 0 and struct.unpack_from("<I", data, 4)[0] == 1
    n, degree = struct.unpack_from("<I", data, 4096 + 4)[0], struct.unpack_from("<H", data, 4096 + 40)[0]
    ncomp = NCOMP[degree]
    table = np.frombuffer(data, np.uint8, n * (44 + 4 * ncomp), 5120).reshape(n, 44 + 4 * ncomp)
    f = lambda lo, hi: np.ascontiguousarray(table[:, lo:hi]).view("<f4")      # noqa: E731
    return {"degree": degree, "c": f(0, 12), "s": f(12, 24), "r": f(24, 40), "rgba": table[:, 40:44].copy(),
            "sh": f(44, 44 + 4 * ncomp) if ncomp else np.zeros((n, 0), np.float32)}


def sh_range(sh, true_minimum=False):
    """SplatBuffer.js:1186-1205: every row, components FRC0 .. FRC22 (the bound is `sc < FRC23 && sc < splat.length`)."""
    lo = hi = None
    falsy = lambda m: m is None or m == 0.0 or m != m      # noqa: E731
    for v in sh[:, :23].astype(np.float64).ravel().tolist():
        if falsy(lo) or v < lo:
            lo = v
        if falsy(hi) or v > hi:
            hi = v
    if true_minimum and sh.size:
        lo = float(np.nanmin(sh.astype(np.float64)))
    return (-1.5 if falsy(lo) else lo), (1.5 if falsy(hi) else hi)


def js_round(x):
    """Math.round: the nearest integer, ties towards +inf."""
    r = np.ceil(x)
    return np.where(r - 0.5 > x, r - 1.0, r)


def or_zero(v):
    """`v || 0` of numbers: NaN and both zeroes become +0."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v) | (v == 0.0), 0.0, v)


def model_encode(rows, level, minimum_alpha=1, block_size=5.0, bucket_size=256, scene_center=(0.0, 0.0, 0.0), mutation=None):
    """-> {"bytes", "order" (the source row stored at each output position), "full", "partial", "bucket_count", "sh_range"}"""
    assert mutation is None or mutation in MUTATIONS
    block_size = float(np.float32(block_size)) or 5.0
    bucket_size = int(bucket_size) or 256
    degree, ncomp = rows["degree"], NCOMP[rows["degree"]]
    kept = np.flatnonzero(rows["rgba"][:, 3].astype(np.int64) >= minimum_alpha)
    n = kept.size
    assert n > 0
    lo, hi = sh_range(rows["sh"], mutation == "true_sh_minimum")
    lo32, hi32 = np.float32(lo), np.float32(hi)
    c64 = rows["c"][kept].astype(np.float64)
    # computeBucketsForUncompressedSplatArray (:1328-1399)
    mn = c64.min(axis=0)
    dims = c64.max(axis=0) - mn
    yb, zb = np.ceil(dims[1] / block_size), np.ceil(dims[2] / block_size)
    blk = np.floor((c64 - mn) / block_size)
    ids = (blk[:, 0] * (yb * zb) + blk[:, 1] * zb + blk[:, 2]).astype(np.int64)
    # A cell's splats fill its open bucket in file order; a bucket that reaches bucket_size is closed.  Full buckets are listed in the
    # order they closed, then the open ones by id (`for (bucketId in obj)`: ascending integer keys).
    by_cell = np.argsort(ids, kind="stable")
    sid = ids[by_cell]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    counts = np.diff(np.r_[starts, n])
    rank = np.arange(n) - np.repeat(starts, counts)
    first_of = np.flatnonzero(rank % bucket_size == 0)                      # (in by_cell order) the first splat of every bucket
    lengths = np.diff(np.r_[first_of, n])
    lengths = np.minimum(lengths, np.repeat(counts, counts)[first_of] - rank[first_of])
    full_b = lengths == bucket_size
    closed_at = by_cell[first_of + lengths - 1]                            # kept position of the splat that closed the bucket
    open_key = by_cell[first_of] if mutation == "open_in_insertion_order" else sid[first_of]
    key = np.where(full_b, closed_at, n + open_key)
    blist = np.argsort(key, kind="stable")
    full, buckets = int(full_b.sum()), len(first_of)
    blen = lengths[blist]
    bucket_of = np.repeat(np.arange(buckets), blen)
    pos = np.repeat(first_of[blist], blen) + (np.arange(n) - np.repeat(np.cumsum(blen) - blen, blen))
    order = by_cell[pos]
    opener = by_cell[first_of[blist]]
    if mutation == "centre_from_id":
        i = ids[opener].astype(np.float64)
        yz = yb * zb if yb * zb else 1.0
        x = np.floor(i / yz)
        y = np.floor((i - x * yz) / (zb if zb else 1.0))
        cell = np.stack([x, y, i - x * yz - y * (zb if zb else 1.0)], axis=1)
    else:
        cell = blk[opener]
    centres = cell * block_size + mn + block_size / 2.0                    # the block centre of the splat that opened the bucket
    if level == 0 and mutation == "no_reorder_at_level0":
        order = np.arange(n)
    src = kept[order]
    # writeSplatDataToSectionBuffer (:1075-1173)
    bps = [44, 24, 24][level] + [4, 2, 1][level] * ncomp
    q = rows["r"][src].astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        qn = q * (1.0 / length)[:, None]
    qn[length == 0.0] = [0.0, 0.0, 0.0, 1.0]                               # Quaternion.normalize of a zero quaternion
    qn[np.isnan(qn)] = np.nan                                              # a typed-array store keeps no particular NaN: the canonical one
    s = or_zero(rows["s"][src])
    sh = or_zero(rows["sh"][src])
    table = np.zeros((n, bps), np.uint8)

    def put(col, a):
        a = np.ascontiguousarray(a)
        table[:, col:col + a.shape[1] * a.itemsize] = a.view(np.uint8).reshape(n, -1)

    if level == 0:
        put(0, rows["c"][src])
        put(12, s.astype(np.float32))
        put(24, qn.astype(np.float32))
    else:
        d = (c64[order] - centres[bucket_of]) * (32767.0 / (block_size * 0.5))
        rounded = np.rint(d) if mutation == "rint_for_round" else js_round(d)
        put(0, np.clip(rounded + 32767.0, 0.0, 65535.0).astype(np.uint16))
        put(6, to_half_three(s))
        put(12, to_half_three(qn))
    col = [40, 20, 20][level]
    put(col, rows["rgba"][src])
    if ncomp:
        if level == 0:
            put(col + 4, sh.astype(np.float32))
        elif level == 1:
            put(col + 4, to_half_three(sh))
        else:
            a, b = float(lo32), float(hi32)
            put(col + 4, np.clip(np.floor((np.clip(sh, a, b) - a) / (b - a) * 255), 0, 255).astype(np.uint8))
    meta = b""
    if level >= 1:
        meta = blen[full:].astype("<u4").tobytes() + centres.astype("<f4").tobytes()
    header = bytearray(4096)
    header[0:2] = bytes([0, 1])
    struct.pack_into("<IIII", header, 4, 1, 1, n, n)
    struct.pack_into("<H", header, 20, level)
    struct.pack_into("<fffff", header, 24, *[float(v) for v in scene_center], lo32, hi32)
    sec = bytearray(1024)
    struct.pack_into("<II", sec, 0, n, n)
    if level >= 1:
        struct.pack_into("<II", sec, 8, bucket_size, buckets)
        struct.pack_into("<f", sec, 16, block_size)
        struct.pack_into("<H", sec, 20, 12)
        struct.pack_into("<I", sec, 24, 32767)
        struct.pack_into("<II", sec, 32, full, buckets - full)
    struct.pack_into("<I", sec, 28, len(meta) + table.size)
    struct.pack_into("<H", sec, 40, degree)
    return {"bytes": bytes(header) + bytes(sec) + meta + table.tobytes(), "order": src.astype(np.uint32), "full": full,
            "partial": buckets - full, "bucket_count": buckets if level >= 1 else 0, "sh_range": (float(lo32), float(hi32)),
            "bytes_per_splat": bps}


# ------------------------------------------------------------------------------------------------ the goldens
def golden():
    z = np.load(os.path.join(GOLDEN, "ksplat_encode_ref.npz"))
    return z, json.loads(z["manifest"].tobytes())["cases"]


_Z, CASES = golden()
_ROWS = {}


def rows_of(name):
    if name not in _ROWS:
        _ROWS[name] = level0_rows(_Z[name + "_file"])
    return _ROWS[name]


def model_of(case, mutation=None):
    return model_encode(rows_of(case["input"]), case["compressionLevel"], case["minimumAlpha"], case["blockSize"], case["bucketSize"],
                        case["sceneCenter"], mutation)


def first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if a.size != b.size:
        return f"sizes {a.size} / {b.size}"
    bad = np.flatnonzero(a != b)
    return None if bad.size == 0 else f"{bad.size} bytes differ, the first at {int(bad[0])}"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_model_equals_the_reference_writer(case):
    assert first_difference(model_of(case)["bytes"], _Z[case["name"] + "_ksplat"].tobytes()) is None


def test_the_cases_show_what_they_are_there_for():
    by_name = {c["name"]: c for c in CASES}
    m = model_of(by_name["exact_l1"])
    assert m["full"] >= 3 and m["partial"] >= 1
    assert model_of(by_name["single_l1"])["order"].tolist() == [137]
    assert model_of(by_name["dropped_l2"])["order"].size == 240
    assert model_of(by_name["zero_sh_l2"])["sh_range"] == (-1.5, 1.5)
    lo, hi = model_of(by_name["dropped_l2"])["sh_range"]
    kept = rows_of("dropped")["rgba"][:, 3] >= 100
    assert lo < rows_of("dropped")["sh"][kept].min() and hi > rows_of("dropped")["sh"][kept].max()      # the extremes sit on dropped rows
    assert model_of(by_name["nonneg_l2"])["sh_range"][0] == 0.015625 and model_of(by_name["nonpos_l2"])["sh_range"][1] == -0.015625
    positive = rows_of("nonneg")["sh"][rows_of("nonneg")["sh"] > 0]
    assert positive.min() < 0.015625                                   # no extreme of the values: what the rule's last reset left
    rows = rows_of("flat")
    assert np.ptp(rows["c"][:, 1]) == 0.0


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_mutation_of_the_model_fails_some_case(mutation):
    failing = [c["name"] for c in CASES if model_of(c, mutation)["bytes"] != _Z[c["name"] + "_ksplat"].tobytes()]
    assert failing, f"no golden case tells the model from its mutation {mutation}"


# gen0 differs from the model in rotation floats only: the reference normalised the PLY's raw quaternion once, a level-0 row was
# normalised when it was stored and is normalised again by the writer.  Bytes that differ, per SH degree of the golden:
GEN0_ROTATION_BYTES = {0: 2, 1: 0, 2: 6}


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_the_model_equals_the_files_the_reference_wrote_from_the_ply(degree):
    z = np.load(os.path.join(GOLDEN, f"assets_ref_sh{degree}.npz"))
    alpha = json.loads(z["manifest"].tobytes())["minimumAlpha"]
    rows = level0_rows(z["ply_ksplat"])
    for level in (1, 2):
        assert first_difference(model_encode(rows, level, alpha)["bytes"], z[f"gen{level}_ksplat"].tobytes()) is None, level
    got = np.frombuffer(model_encode(rows, 0, alpha)["bytes"], np.uint8)
    want = z["gen0_ksplat"]
    assert got.size == want.size and np.array_equal(got[:5120], want[:5120])
    bps = 44 + 4 * NCOMP[degree]
    bad = np.flatnonzero(got[5120:] != want[5120:])
    assert ((bad % bps >= 24) & (bad % bps < 40)).all(), "a byte outside the rotation floats differs"
    print(f"degree {degree}: {bad.size} rotation bytes differ")
    assert bad.size == GEN0_ROTATION_BYTES[degree]


# ------------------------------------------------------------------------------------------------ the library, without a device
def params(level=1, alpha=1, bucket=256, block=5.0, centre=(0.0, 0.0, 0.0), flags=0):
    return _lib.KsplatParams(level, alpha, bucket, block, (C.c_float * 3)(*centre), flags)


def open_asset(data, fmt=_lib.GS_ASSET_KSPLAT):
    lib, h = g.load(), C.c_void_p()
    buf = (C.c_char * len(data)).from_buffer_copy(bytes(data))
    assert lib.gs_asset_open(buf, len(data), fmt, 2, C.byref(h)) == 0
    return h


def encode_status(asset, p):
    out = C.c_void_p()
    st = g.load().gs_asset_encode_ksplat(None, asset, C.byref(p), C.byref(out), None)
    assert not out.value
    return st


def test_the_entry_points_are_declared_exported_and_typed():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+gs_asset_encode_ksplat\s*\(([^)]*)\)\s*;", code)
    assert decl and [p.strip().split("*")[0].strip() for p in decl.group(1).split(",")] == ["gs_context", "gs_asset", "const gs_ksplat_params",
                                                                                           "gs_asset", "uint32_t"]
    assert re.search(r"\bint\s+gs_asset_bytes\s*\(\s*gs_asset\*\s*\w+,\s*const void\*\*\s*\w+,\s*uint64_t\*\s*\w+\)\s*;", code)
    fields = re.search(r"typedef struct gs_ksplat_params \{(.*?)\} gs_ksplat_params;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[3\])?;", fields) == [f[0] for f in _lib.KsplatParams._fields_]
    assert C.sizeof(_lib.KsplatParams) == 32
    lib = g.load()
    for name in ("gs_asset_encode_ksplat", "gs_asset_bytes"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 5 and lib.gs_abi_version() == 5
    assert callable(assets.SplatAsset.encode_ksplat) and callable(assets.SplatAsset.to_bytes)


def test_the_refusals_that_need_no_device():
    lib = g.load()
    level0 = open_asset(_Z["sh1_file"])
    try:
        assert encode_status(level0, params(level=3)) == _lib.GS_ERR_INVALID
        assert encode_status(level0, params(flags=1)) == _lib.GS_ERR_INVALID
        for block in (-1.0, float("inf"), float("nan")):
            assert encode_status(level0, params(block=block)) == _lib.GS_ERR_INVALID, block
        assert encode_status(level0, params(bucket=65536)) == _lib.GS_ERR_INVALID
        matrix = (C.c_double * 16)(*np.eye(4).ravel())
        assert lib.gs_asset_set_transform(level0, matrix) == 0
        assert encode_status(level0, params()) == _lib.GS_ERR_INVALID
        assert b"transform" in lib.gs_last_error()
        assert lib.gs_asset_set_transform(level0, None) == 0
        # every parameter is fine now: what is missing is the device
        assert encode_status(level0, params()) == _lib.GS_ERR_INVALID and b"context" in lib.gs_last_error()
        data, size = C.c_void_p(), C.c_uint64()
        assert lib.gs_asset_bytes(level0, C.byref(data), C.byref(size)) == _lib.GS_ERR_INVALID      # no encoder result
    finally:
        lib.gs_asset_close(level0)
    for name in ("sh1_l1", "sh1_l2"):
        quantised = open_asset(_Z[name + "_ksplat"])
        try:
            assert encode_status(quantised, params()) == _lib.GS_ERR_UNSUPPORTED, name
        finally:
            lib.gs_asset_close(quantised)
    empty, _ = assets.write_ksplat(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4)), np.zeros((0, 4), np.uint8))
    none = open_asset(empty)
    try:
        assert encode_status(none, params()) == _lib.GS_ERR_INVALID
    finally:
        lib.gs_asset_close(none)


class Layout(C.Structure):
    _fields_ = [("bytes_per_splat", C.c_uint32), ("bucket_count", C.c_uint32), ("partial_off", C.c_uint64), ("buckets_off", C.c_uint64),
                ("rows_off", C.c_uint64), ("storage_bytes", C.c_uint64), ("total_bytes", C.c_uint64)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_host_layout_has_the_models_sizes_and_offsets(case):
    lib = g.load()
    lib.gs_debug_ksplat_layout.restype = C.c_int
    lib.gs_debug_ksplat_layout.argtypes = [C.c_uint32] * 5 + [C.POINTER(Layout)]
    m, level = model_of(case), case["compressionLevel"]
    n, degree = m["order"].size, rows_of(case["input"])["degree"]
    lay = Layout()
    assert lib.gs_debug_ksplat_layout(level, degree, n, m["full"], m["partial"], C.byref(lay)) == 0
    meta = 4 * m["partial"] if level else 0
    assert lay.bytes_per_splat == m["bytes_per_splat"] and lay.bucket_count == m["bucket_count"]
    assert (lay.partial_off, lay.buckets_off, lay.rows_off) == (5120, 5120 + meta, 5120 + meta + 12 * m["bucket_count"])
    assert lay.total_bytes == len(m["bytes"]) and lay.storage_bytes == len(m["bytes"]) - 5120
    assert lay.storage_bytes == struct.unpack_from("<I", m["bytes"], 4096 + 28)[0]
    assert lib.gs_debug_ksplat_layout(3, 0, 1, 0, 1, C.byref(lay)) == _lib.GS_ERR_INVALID
