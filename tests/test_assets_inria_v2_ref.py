"""The native INRIA-v2 codebook PLY reader (csrc/assets.hip: the codebook decoded once at open, rows through the shared row arithmetic
of csrc/asset_internal.hpp) against the reference's own parser, executed: tests/golden/assets_inria_v2_ref.npz holds seeded files and
what INRIAV2PlyParser.parseToUncompressedSplat + the level-0 store + the SplatBuffer fills return for them, row by row in file order
(tests/tools/make_inria_v2_golden.py).

Values are compared BITWISE where neither side is NaN, and the NaN masks must be equal (same_bits of tests/test_assets_formats_ref.py).
No tolerance anywhere."""
import numpy as np
import pytest

import asset_inria_v2_cases as VC
from gaussiansplats3d_amd import assets
from test_assets_formats_ref import same_bits


@pytest.mark.parametrize("name", VC.cases())
def test_fills_equal_the_reference(name):
    g, _ = VC.golden()
    data, fmt, degree, entry = VC.case(name)
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
        if name.startswith("v2_hostile"):
            assert not np.array_equal(g[f"{name}_rgba1"], g[f"{name}_rgba40"]), "the case has no alpha between 1 and 39"
        same_bits(f1["scales"], g[f"{name}_scales"], "scales")
        same_bits(f1["rotations"], g[f"{name}_rotations"], "rotations")
        if entry["ncoef"]:
            same_bits(f1["sh_f16"], g[f"{name}_sh"], "sh_f16")
        else:
            assert f1["sh_f16"] is None and f1["sh_u8"] is None
        a.set_transform(VC.matrix())
        with np.errstate(all="ignore"):
            t32, t16 = a.fill(1, False), a.fill(1, True)
        same_bits(t32["centers"], g[f"{name}_xf_centers"], "transformed centres")
        same_bits(t32["cov"], g[f"{name}_xf_cov32"], "transformed cov")
        same_bits(t16["cov_f16"], g[f"{name}_xf_cov16"], "transformed cov_f16")
    finally:
        a.close()


def test_the_golden_holds_what_it_is_for():
    """NaN rows exist in v2_hostile alone and are few; its four opacity entries sit on both sides of minimum alpha 40; v2_bare shows what
    the reference makes of absent field groups."""
    g, man = VC.golden()
    assert sorted({e["file"] for e in man["cases"]}) == ["v2_bare_file", "v2_hostile_file", "v2_sh0_file", "v2_sh1_file", "v2_sh2_file",
                                                         "v2_sh3_file"]
    assert [(e["name"], e["shDegree"]) for e in man["cases"] if e["file"] in ("v2_sh2_file", "v2_sh3_file")] == \
        [("v2_sh2_d2", 2), ("v2_sh2_d0", 0), ("v2_sh3_d2", 2), ("v2_sh3_d1", 1)]
    for entry in man["cases"]:
        assert entry["splatCount"] == 600
        if entry["file"] == "v2_hostile_file":
            assert 0 < entry["splatsWithNaN"] < 0.05 * entry["splatCount"], entry
        else:
            assert entry["splatsWithNaN"] == 0, entry
    assert g["v2_hostile_d2_rgba1"][100:104, 3].tolist() == [0, 39, 40, 255]
    assert g["v2_hostile_d2_rgba40"][100:104, 3].tolist() == [0, 0, 40, 255]
    c = g["v2_hostile_d2_centers"]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c == 65504.0).any()
    assert ((c == 0) & np.signbit(c)).any() and ((c != 0) & (np.abs(c) < 6.2e-5)).any(), "no -0 / subnormal half among the centres"
    assert np.isinf(g["v2_hostile_d2_scales"]).any() and (g["v2_hostile_d2_scales"] == 0).any()
    assert (g["v2_bare_d0_scales"] == np.float32(0.01)).all() and not g["v2_bare_d0_rgba1"].any()
