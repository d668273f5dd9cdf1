"""gs_asset_open on .spz files: the library's own gzip reader (csrc/spz_container.hpp: every way zlib lays a stream out, every
optional header field) and what is refused, each by name in gs_last_error (GS_ERR_INVALID, `out` left NULL); a seeded damage
run; format detection and the constants' mirrors; the writer of gaussiansplats3d_amd.assets through the reader."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

from gaussiansplats3d_amd import _lib as L
from gaussiansplats3d_amd import assets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic(n=300, degree=1, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)), rng.normal(-3.0, 0.5, size=(n, 3)), rng.normal(size=(n, 4)), rng.random((n, 4)),
            rng.normal(0.0, 0.3, size=(n, 3 * (0, 3, 8, 15)[degree])) if degree else None)


def stream(n=300, degree=1, **kw):
    return assets.spz_stream(*synthetic(n, degree), **kw)


def member(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flags=0, extra=b"", name=b"", comment=b"", crc=None, isize=None):
    """A gzip member around `payload`: raw deflate from zlib, the RFC 1952 header and trailer written here."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        body = co.compress(payload) + co.flush()
    else:
        body = co.compress(payload[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(payload[flush_at:]) + co.flush()
    head = bytes([0x1F, 0x8B, 8, flags]) + struct.pack("<IBB", 0, 0, 255)
    if flags & 4:
        head += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        head += name + b"\0"
    if flags & 16:
        head += comment + b"\0"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) & 0xFFFFFFFF if isize is None else isize)


def open_status(data, fmt=L.GS_ASSET_SPZ):
    lib = L.load()
    handle = C.c_void_p(0xDEAD)
    buf = (C.c_char * max(len(data), 1)).from_buffer_copy(data or b"\0")
    st = lib.gs_asset_open(buf, len(data), fmt, 2, C.byref(handle))
    if st == L.GS_OK:
        lib.gs_asset_close(handle)
    return st, handle.value


def refused(data, *words):
    """GS_ERR_INVALID, `out` NULL, and every word in the message."""
    st, handle = open_status(data)
    message = L.load().gs_last_error().decode()
    assert st == L.GS_ERR_INVALID and handle is None, (st, handle)
    for w in words:
        assert w in message, (w, message)
    return message


def filled(data, degree=2):
    a = assets.SplatAsset(data, "spz", degree)
    try:
        f = a.fill(1, False, want_scale_rotation=True)
        return {k: f[k] for k in ("centers", "cov", "rgba", "sh_f16", "scales", "rotations")}
    finally:
        a.close()


def assert_same_fill(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the inflate, through the public entry
LAYOUTS = {
    "stored": dict(level=0),
    "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "level1": dict(level=1),
    "level6": dict(level=6),
    "level9": dict(level=9),
    "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(level=6, strategy=zlib.Z_RLE),
    "two_blocks": dict(level=6, flush_at=3000),
    "stored_two_blocks": dict(level=0, flush_at=17),
    "flush_inside_the_header": dict(level=6, flush_at=7),
    "fextra": dict(flags=4, extra=b"\x41\x42\x04\x00abcd"),
    "fextra_empty": dict(flags=4),
    "fname": dict(flags=8, name=b"scene.spz"),
    "fcomment": dict(flags=16, comment=b"a comment"),
    "fhcrc": dict(flags=2),
    "every_field": dict(flags=2 | 4 | 8 | 16, extra=b"xy", name=b"n", comment=b""),
}


@pytest.fixture(scope="module")
def baseline():
    payload = stream()
    return payload, filled(assets.write_spz(*synthetic()))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_deflate_layout_and_header_field_fills_identically(baseline, layout):
    payload, want = baseline
    data = member(payload, **LAYOUTS[layout])
    assert zlib.decompress(data, 31) == payload                      # the member is what it claims to be
    assert_same_fill(filled(data), want)


def test_a_compressible_stream_with_long_matches(baseline):
    """Constant planes: matches of length 258 at distance 1 and overlapping copies, in dynamic and in fixed blocks."""
    n = 5000
    z = np.zeros((n, 3))
    payload = assets.spz_stream(z, z - 3.0, np.tile([1.0, 0, 0, 0], (n, 1)), np.full((n, 4), 0.5), np.zeros((n, 45)))
    for kw in (dict(level=9), dict(level=6, strategy=zlib.Z_FIXED)):
        data = member(payload, **kw)
        assert len(data) < len(payload) // 50
        f = filled(data)
        assert f["centers"].shape == (n, 3) and not f["centers"].any() and (f["rgba"] == f["rgba"][0]).all()


def test_zero_splats():
    payload = struct.pack("<IIIBBBB", 1347635022, 2, 0, 3, 12, 0, 0)
    assert open_status(member(payload))[0] == L.GS_OK
    refused(member(payload + b"\0"), "more bytes than the header implies")


# ------------------------------------------------------------------------------------------------ refusals: gzip
def test_wrong_crc_and_isize(baseline):
    payload, _ = baseline
    refused(member(payload, crc=zlib.crc32(payload) ^ 1), "CRC-32")
    refused(member(payload, isize=len(payload) + 1), "ISIZE")
    refused(member(payload, flags=2)[:10] + b"\0\0" + member(payload, flags=2)[12:], "CRC-16")


def test_trailing_bytes(baseline):
    payload, _ = baseline
    good = member(payload)
    refused(good + b"\0", "trailing bytes")
    refused(good + good, "trailing bytes")                               # a second member


def test_not_gzip_or_not_deflate(baseline):
    payload, _ = baseline
    good = member(payload)
    refused(payload, "1f 8b")                                            # the bare stream
    refused(b"", "shorter than a gzip header")
    refused(good[:2] + b"\x07" + good[3:], "not deflate")
    refused(good[:3] + b"\x20" + good[4:], "reserved gzip flag")
    refused(member(payload, flags=0)[:10] + b"\x07" + b"\0" * 20, "reserved type 3")    # BFINAL = 1, BTYPE = 3


def test_truncation_at_every_byte():
    """A small file (header + 3 splats with SH), stored and compressed, every optional field present: no prefix opens."""
    payload = stream(3, 1)
    for kw in (dict(level=0), dict(level=9), dict(level=6, strategy=zlib.Z_FIXED)):
        good = member(payload, flags=2 | 4 | 8 | 16, extra=b"xy", name=b"n", comment=b"c", **kw)
        assert open_status(good)[0] == L.GS_OK
        for cut in range(len(good)):
            st, handle = open_status(good[:cut])
            assert st == L.GS_ERR_INVALID and handle is None, (kw, cut)


def test_one_byte_more_or_less_than_the_header_implies(baseline):
    payload, _ = baseline
    for kw in (dict(level=0), dict(level=6), dict(level=6, strategy=zlib.Z_FIXED)):
        refused(member(payload + b"\0", **kw), "more bytes than the header implies")
        refused(member(payload[:-1], **kw), "incorrect size")
    refused(member(payload[:15]), "shorter than the 16-byte SPZ header")
    refused(member(b""), "shorter than the 16-byte SPZ header")


def test_a_match_before_the_start_of_the_output():
    # fixed block: BFINAL 1, BTYPE 01, then length symbol 257 (7 bits 0000001) + distance symbol 0 (5 bits): a match at size 0
    bits = "1" + "10" + "0000001" + "00000"
    bits += "0" * (-len(bits) % 8)
    body = bytes(int(bits[k:k + 8][::-1], 2) for k in range(0, len(bits), 8))
    head = bytes([0x1F, 0x8B, 8, 0]) + struct.pack("<IBB", 0, 0, 255)
    refused(head + body + b"\0" * 8, "before the start of the output")


# ------------------------------------------------------------------------------------------------ refusals: the container
def with_header(payload, **fields):
    magic, version, n, degree, bits, flags, reserved = struct.unpack_from("<IIIBBBB", payload, 0)
    h = dict(magic=magic, version=version, n=n, degree=degree, bits=bits, flags=flags, reserved=reserved)
    h.update(fields)
    return struct.pack("<IIIBBBB", h["magic"], h["version"], h["n"], h["degree"], h["bits"], h["flags"], h["reserved"]) + payload[16:]


def test_container_refusals(baseline):
    payload, _ = baseline
    refused(member(with_header(payload, magic=1347635021)), "wrong magic")
    refused(member(with_header(payload, version=0)), "version not supported")
    refused(member(with_header(payload, version=3)), "version not supported")
    refused(member(with_header(payload, n=10_000_001)), "too many points")
    refused(member(with_header(payload, n=0xFFFFFFFF)), "too many points")
    refused(member(with_header(payload, degree=4)), "unsupported SH degree")
    refused(member(with_header(payload, n=299)), "more bytes than the header implies")
    refused(member(with_header(payload, n=301)), "incorrect size")
    refused(member(with_header(payload, version=1)), "more bytes than the header implies")   # 6-byte positions: the planes are too long
    refused(member(with_header(payload, degree=0)), "more bytes than the header implies")
    refused(member(with_header(payload, degree=2)), "incorrect size")


def test_flags_and_reserved_are_dropped(baseline):
    payload, want = baseline
    assert_same_fill(filled(member(with_header(payload, flags=1))), want)          # antialiased: parsed and dropped
    assert_same_fill(filled(member(with_header(payload, flags=0xFE, reserved=0xFF))), want)


def test_info(baseline):
    payload, _ = baseline
    for want_degree, got_degree in ((0, 0), (1, 1), (2, 1), (3, 1)):
        a = assets.SplatAsset(member(payload), "spz", want_degree)
        i = a.info
        assert (i.splat_count, i.sh_degree, i.compression_level, i.sh_level) == (300, got_degree, 0, 1)
        assert tuple(i.scene_center) == (0.0, 0.0, 0.0) and (i.sh_min, i.sh_max) == (-1.5, 1.5)
        a.close()
    a = assets.SplatAsset(member(stream(50, 3)), "spz", 3)                 # a degree-3 file gives degree 2
    assert a.info.sh_degree == 2
    a.close()


# ------------------------------------------------------------------------------------------------ damage
def test_200_single_byte_flips(baseline):
    """Each damaged file is refused or opens and fills (the CRC-32 catches a flip in the deflate body; a flip in MTIME / XFL / OS
    changes nothing).  Whichever happens the process goes on and a good file still opens."""
    payload, want = baseline
    good = member(payload, level=6, flags=8, name=b"scene.spz")
    rng = np.random.default_rng(11)
    outcomes = {"refused": 0, "opened": 0}
    for _ in range(200):
        bad = bytearray(good)
        at = int(rng.integers(0, len(bad)))
        bad[at] ^= 1 << int(rng.integers(0, 8))
        st, handle = open_status(bytes(bad))
        if st == L.GS_OK:
            f = filled(bytes(bad))
            assert f["centers"].shape == (300, 3)
            outcomes["opened"] += 1
        else:
            assert st == L.GS_ERR_INVALID and handle is None
            outcomes["refused"] += 1
    assert outcomes["refused"] > 150, outcomes
    assert_same_fill(filled(good), want)


# ------------------------------------------------------------------------------------------------ mirrors and detection
def test_the_constant_in_header_mirror_and_shim():
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    m = re.search(r"enum\s*\{\s*GS_ASSET_SPZ\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == L.GS_ASSET_SPZ == 4
    assert "#define GS_ASSET_SPZ" not in header
    js = open(os.path.join(ROOT, "node", "gsplat.js")).read()
    m = re.search(r"const AssetFormat = \{([^}]*)\}", js)
    got = {k.strip(): int(v) for k, v in (kv.split(":") for kv in m.group(1).split(","))}
    assert got == {"ply": L.GS_ASSET_PLY, "ksplat": L.GS_ASSET_KSPLAT, "splat": L.GS_ASSET_SPLAT, "spz": L.GS_ASSET_SPZ}
    assert assets.SplatAsset.FORMATS["spz"] == L.GS_ASSET_SPZ


def test_detection(tmp_path, baseline):
    _, want = baseline
    data = assets.write_spz(*synthetic())
    assert data[:2] == b"\x1f\x8b"
    a = assets.SplatAsset(data)                                          # fmt=None: the gzip magic
    assert a.info.splat_count == 300
    a.close()
    path = str(tmp_path / "Scene.SPZ")
    open(path, "wb").write(data)
    out = assets.load(path, spherical_harmonics_degree=2)
    assert np.array_equal(out["centers"], want["centers"]) and np.array_equal(out["sh_f16"], want["sh_f16"])
    with pytest.raises(ValueError):
        assets.SplatAsset(bytes(64), fmt="spz")                          # refused in Python: no gzip magic
    st, _ = open_status(data, L.GS_ASSET_KSPLAT)
    assert st == L.GS_ERR_INVALID                                        # the library does not guess: the format is the caller's


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("version,bits,degree", [(2, 12, 0), (2, 12, 3), (2, 8, 1), (2, 16, 2), (1, 12, 2)])
def test_write_spz_round_trips(version, bits, degree):
    """Within one quantisation step per field, each step taken from the format, not from the output."""
    n = 300
    c, ls, q, rgba, sh = synthetic(n, degree)
    a = assets.SplatAsset(assets.write_spz(c, ls, q, rgba, sh, version=version, fractional_bits=bits), fmt="spz")
    f = a.fill(1, False, want_scale_rotation=True)
    a.close()
    assert (a.info.splat_count, a.info.sh_degree) == (n, min(degree, 2))
    if version == 2:
        assert np.abs(f["centers"].astype(np.float64) - c).max() <= 2.0 ** -bits / 2 + 2.0 ** -22    # half a step + the fp32 store below 8
    else:
        assert np.array_equal(f["centers"], c.astype(np.float16).astype(np.float32))               # halves widen exactly
    assert np.abs(np.log(f["scales"].astype(np.float64)) - ls).max() <= 1.0 / 16                    # the step of the scale byte
    # x, y, z are coded as bytes of step 1 / 127.5 and w is rebuilt from them, so the file's quaternion is a unit one up to
    # rounding and the normalisations move x, y, z by far less than a step; w itself has no bounded step near 0
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    qn = qn * np.where(qn[:, :1] < 0, -1.0, 1.0)
    got = f["rotations"].astype(np.float64)                                                       # x, y, z, w with w >= 0
    assert np.abs(got[:, :3] - qn[:, 1:]).max() <= 1.0 / 127.5 and (got[:, 3] >= 0).all()
    alpha = np.floor(rgba[:, 3] * 255 + 0.5)
    assert np.array_equal(f["rgba"][:, 3], np.where(alpha >= 1, alpha, 0).astype(np.uint8))
    # colour byte steps are 1 / 255 of the wire value, stretched by SH_C0 / 0.15 on the way out, floor'ed onto 0..255
    step = 0.28209479177387814 / 0.15
    assert np.abs(f["rgba"][:, :3].astype(np.float64) - np.clip(rgba[:, :3] * 255, 0, 255)).max() <= step / 2 + 1.0
    if degree:
        dim = (0, 3, 8, 15)[degree]
        per = sh.reshape(n, 3, dim)
        want = np.concatenate([per[:, :, lo:hi].transpose(0, 2, 1).reshape(n, -1) for lo, hi in ((0, 3), (3, 8))[:min(degree, 2)]], axis=1)
        got_sh = np.asarray(f["sh_f16"]).view(np.float16).astype(np.float64)
        assert np.abs(got_sh - np.clip(want, -1.0, 127.0 / 128)).max() <= 1.0 / 256 + 2.0 ** -11       # half a byte step + the half's truncation below 1
