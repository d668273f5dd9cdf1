"""The native .splat and PlayCanvas compressed PLY readers (csrc/assets.hip over the shared row arithmetic of
csrc/asset_internal.hpp) against the reference's own parsers, executed: tests/golden/assets_formats_ref.npz holds seeded
files and what SplatParser / PlyParser + the SplatBuffer fills return for them (tests/tools/make_formats_golden.py).

Values are compared BITWISE where neither side is NaN, and the NaN masks must be equal: a typed-array store keeps no
particular NaN, so a NaN's bits say nothing.  No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

import asset_formats_cases as FC
from gaussiansplats3d_amd import assets


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}"
    if got.dtype == np.uint16:                        # half bits: NaN = exponent 31 with a mantissa
        nan_g, nan_r = (got & 0x7FFF) > 0x7C00, (ref & 0x7FFF) > 0x7C00
    elif got.dtype.kind == "f":
        nan_g, nan_r = np.isnan(got), np.isnan(ref)
    else:
        nan_g = nan_r = np.zeros(got.shape, bool)
    assert np.array_equal(nan_g, nan_r), f"{what}: the NaN masks differ at {np.argwhere(nan_g != nan_r)[:5].tolist()}"
    raw = {2: np.uint16, 4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = (got.view(raw) != ref.view(raw)) & ~nan_g
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[:5].tolist()}"


@pytest.mark.parametrize("name", FC.cases())
def test_fills_equal_the_reference(name):
    g, _ = FC.golden()
    data, fmt, degree, entry = FC.case(name)
    a = assets.SplatAsset(data, fmt, degree)
    try:
        info = a.info
        assert (info.splat_count, info.sh_degree, info.compression_level, info.sh_level) == (entry["splatCount"], entry["shDegree"], 0, 1)
        with np.errstate(all="ignore"):
            f1 = a.fill(1, False, want_scale_rotation=True)
            f40 = a.fill(40, True)
        same_bits(f1["centers"], g[f"{name}_centers"], "centres")
        same_bits(f1["cov"], g[f"{name}_cov32"], "cov")
        same_bits(f40["cov_f16"], g[f"{name}_cov16"], "cov_f16")
        same_bits(f1["rgba"], g[f"{name}_rgba1"], "rgba at minimum alpha 1")
        same_bits(f40["rgba"], g[f"{name}_rgba40"], "rgba at minimum alpha 40")
        assert not np.array_equal(g[f"{name}_rgba1"], g[f"{name}_rgba40"]), "the case has no alpha between 1 and 39"
        same_bits(f1["scales"], g[f"{name}_scales"], "scales")
        same_bits(f1["rotations"], g[f"{name}_rotations"], "rotations")
        if entry["ncoef"]:
            same_bits(f1["sh_f16"], g[f"{name}_sh"], "sh_f16")
        else:
            assert f1["sh_f16"] is None and f1["sh_u8"] is None
        a.set_transform(FC.matrix())
        with np.errstate(all="ignore"):
            t32, t16 = a.fill(1, False), a.fill(1, True)
        same_bits(t32["centers"], g[f"{name}_xf_centers"], "transformed centres")
        same_bits(t32["cov"], g[f"{name}_xf_cov32"], "transformed cov")
        same_bits(t16["cov_f16"], g[f"{name}_xf_cov16"], "transformed cov_f16")
    finally:
        a.close()


def test_the_golden_holds_what_it_is_for():
    """NaN rows exist but are few, and the colour lerps of the extremes cases reach the rails the .5 rows were written for."""
    g, man = FC.golden()
    for entry in man["cases"]:
        if entry["fmt"] == "ply":
            assert 0 < entry["splatsWithNaN"] < 0.05 * entry["splatCount"], entry
    assert (g["pc_sh0_ext_d0_rgba1"][256:296:2, 0] == 128).all()        # Math.round(127.5)
    assert (g["pc_sh0_ext_d0_rgba1"][256:296:2, 1] == 0).all()          # Math.round(-127.5) = -127, clamped
    assert (g["pc_sh0_ext_d0_rgba1"][256:296:2, 2] == 1).all()          # Math.round(0.5 / 255 as fp32 * 255) on its .5


def test_an_inria_v1_ply_is_still_read_as_one():
    """Detection did not move INRIA-v1: the reference-written PLY of assets_ref_sh2.npz still fills to its own golden."""
    g = np.load(os.path.join(FC.GOLDEN, "assets_ref_sh2.npz"))
    man = json.loads(bytes(g["manifest"]).decode())
    a = assets.SplatAsset(bytes(g["ply_bytes"]), "ply", man["shDegree"])
    try:
        f = a.fill(1, False)
        same_bits(f["centers"], g["ply_centers"], "centres")
        same_bits(f["cov"], g["ply_cov32"], "cov")
        same_bits(f["rgba"], g["ply_rgba"], "rgba")
        same_bits(f["sh_f16"], g["ply_sh"], "sh")
    finally:
        a.close()
