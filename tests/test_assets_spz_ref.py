"""The native .spz reader (the gzip reader and container of csrc/spz_container.hpp, csrc/assets.hip over the shared row
arithmetic of csrc/asset_internal.hpp) against the reference's own SpzLoader, executed: tests/golden/assets_spz_ref.npz holds
seeded files and what SpzLoader.loadFromFileData(.., optimizeSplatData = false, degree) + the SplatBuffer fills return for
them (tests/tools/make_spz_golden.py).

Values are compared BITWISE where neither side is NaN, and the NaN masks must be equal (only the version-1 file's half
positions carry NaNs): a typed-array store keeps no particular NaN.  No tolerance anywhere."""
import gzip
import struct

import numpy as np
import pytest

import asset_spz_cases as SC
from gaussiansplats3d_amd import assets
from test_assets_formats_ref import same_bits


@pytest.mark.parametrize("name", SC.cases())
def test_fills_equal_the_reference(name):
    data, fmt, degree, entry = SC.case(name)
    ref = lambda key: SC.array(name, key)                        # noqa: E731
    a = assets.SplatAsset(data, fmt, degree)
    try:
        info = a.info
        assert (info.splat_count, info.sh_degree, info.compression_level, info.sh_level) == (entry["splatCount"], entry["shDegree"], 0, 1)
        assert tuple(info.scene_center) == (0.0, 0.0, 0.0) and (info.sh_min, info.sh_max) == (-1.5, 1.5)
        with np.errstate(all="ignore"):
            f1 = a.fill(1, False, want_scale_rotation=True)
            f40 = a.fill(40, True)
        same_bits(f1["centers"], ref("centers"), "centres")
        same_bits(f1["cov"], ref("cov32"), "cov")
        same_bits(f40["cov_f16"], ref("cov16"), "cov_f16")
        same_bits(f1["rgba"], ref("rgba1"), "rgba at minimum alpha 1")
        same_bits(f40["rgba"], ref("rgba40"), "rgba at minimum alpha 40")
        assert not np.array_equal(ref("rgba1"), ref("rgba40")), "the case has no alpha between 1 and 39"
        same_bits(f1["scales"], ref("scales"), "scales")
        same_bits(f1["rotations"], ref("rotations"), "rotations")
        if entry["ncoef"]:
            same_bits(f1["sh_f16"], ref("sh"), "sh_f16")
        else:
            assert f1["sh_f16"] is None and f1["sh_u8"] is None
        a.set_transform(SC.matrix())
        with np.errstate(all="ignore"):
            t32, t16 = a.fill(1, False), a.fill(1, True)
        same_bits(t32["centers"], ref("xf_centers"), "transformed centres")
        same_bits(t32["cov"], ref("xf_cov32"), "transformed cov")
        same_bits(t16["cov_f16"], ref("xf_cov16"), "transformed cov_f16")
        if entry["ncoef"]:
            same_bits(t32["sh_f16"], ref("xf_sh"), "transformed sh_f16")
    finally:
        a.close()


def planes_of(name):
    """(header fields, {plane: uint8 [n, stride]}) of a golden file's inflated stream."""
    stream = gzip.decompress(SC.case(name)[0])
    magic, version, n, degree, bits, flags, reserved = struct.unpack_from("<IIIBBBB", stream, 0)
    out, at = {}, 16
    for plane, stride in (("positions", 9 if version == 2 else 6), ("alphas", 1), ("colours", 3), ("scales", 3), ("rotations", 3),
                          ("sh", 3 * (0, 3, 8, 15)[degree])):
        out[plane] = np.frombuffer(stream, np.uint8, stride * n, at).reshape(n, stride)
        at += stride * n
    assert at == len(stream)
    return (version, n, degree, bits), out


def test_the_golden_holds_what_it_is_for():
    man = SC.golden()[1]
    reads = {(c["base"], c["degree"]): c["shDegree"] for c in man["cases"]}
    for degree in range(4):                                      # version 2 at every file degree, read at every output degree
        for out_degree in range(3):
            assert reads[(f"v2_sh{degree}", out_degree)] == min(degree, out_degree)
    assert [planes_of(f"v2_fb{b}_d0")[0][3] for b in (0, 31, 40)] == [0, 31, 40]
    assert planes_of("v2_sh3_d2")[0] == (2, 600, 3, 12)
    # fractionalBits 31: 1 << 31 is negative in JavaScript, so every centre has the opposite sign of its fixed-point value
    _, p = planes_of("v2_fb31_d0")
    fixed = p["positions"].reshape(600, 3, 3).astype(np.int64)
    fixed = fixed[..., 0] | (fixed[..., 1] << 8) | (fixed[..., 2] << 16)
    fixed = np.where(fixed & 0x800000, fixed - (1 << 24), fixed)
    c = SC.array("v2_fb31_d0", "centers")
    assert (fixed != 0).all() and (np.sign(c) == -np.sign(fixed)).all()
    # fractionalBits 40 reads as 8
    _, p = planes_of("v2_fb40_d0")
    fixed = p["positions"].reshape(600, 3, 3).astype(np.int64)
    fixed = fixed[..., 0] | (fixed[..., 1] << 8) | (fixed[..., 2] << 16)
    fixed = np.where(fixed & 0x800000, fixed - (1 << 24), fixed)
    assert np.array_equal(SC.array("v2_fb40_d0", "centers"), (fixed / 256.0).astype(np.float32))
    # version 1: the halves the case is for
    (version, _, _, _), p = planes_of("v1_sh1_d1")
    halves = p["positions"].copy().view("<u2").reshape(-1)
    assert version == 1 and {0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7C00, 0xFC00, 0x7C01, 0xFE00} <= set(halves.tolist())
    c = SC.array("v1_sh1_d1", "centers")
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c[np.signbit(c)] == 0).any()
    # the exhaustive file
    _, p = planes_of("exhaustive_d1")
    for plane in ("scales", "colours", "alphas", "sh"):
        assert len(np.unique(p[plane])) == 256, plane
    c = SC.array("exhaustive_d1", "centers")
    assert {-2048.0, 0.0} <= set(c.reshape(-1).tolist()) and np.float32((2 ** 23 - 1) / 4096.0) in c
    r = p["rotations"].astype(np.float64) / 127.5 - 1.0
    sq = (r * r).sum(axis=1)
    assert (sq < 1).any() and (sq > 1).any() and (p["rotations"] == 255).all(axis=1).any()
