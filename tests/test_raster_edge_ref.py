"""CPU tier of the DESIGNED edge cases of the vertex stage (tests/raster_edge_cases.py): covariances whose 2D off-diagonal term is exactly
0 (the last bit of `traceOver2 * traceOver2 - D` decides whether the reference's shader draws them), ladders of adjacent floats across
every threshold that decides a splat, non-finite and degenerate inputs.  tests/golden/raster_edge_ref.npz holds what the reference's
own GLSL computes for them (oracle/make_golden_raster.py --edges); no tolerance applies to a verdict.

  census        counted on the shader's outputs alone while the golden was made, recorded in the file, recounted and asserted here: about
                half of every knife-edge sub-case is drawn and half is left NaN, every ladder's verdict changes exactly once and, where
                its rungs are adjacent floats, between two of them; every drawn splat is large and inside enough that the engine's
                thin-or-outside drop cannot apply (so the GPU tier may demand on_screen == drawn)
  C oracle      oracle.project gives the shader's verdict on EVERY splat; what is drawn passes check_oracle_projection unchanged
  restatement   raster_edge_ref.verdicts (numpy float32, one rounding per operation) equals the shader's verdicts on every splat
  mutations     each mistake the restatement can be made to make changes a verdict, in the class named for it: the cases see it.

Two thresholds of the issue's list decide nothing and have no mutation: the 1.2 w test on z is implied by GL's clip of the quad's depth
(w > 0 and z < -1.2 w give z / w < -1; w <= 0 fails an x or y test or leaves NaN), and the floor 0.1 moved one ulp DOWN changes no
float anywhere, because sqrt of the float below 0.1f is sqrt(0.1f) again.  The size cap and the fade's step and clamp are continuous at
their thresholds: nothing is decided there and a swapped strictness changes no float, but their ladders still pin the float at which
each sets in (test_c_oracle_caps_and_fades_at_the_shaders_floats)."""
import json
import os

import numpy as np
import pytest

import raster_edge_cases as rec
import raster_edge_ref
from oracle.make_golden_raster import edge_census, shader_verdicts
from test_raster_ref import _oracle_camera, check_oracle_projection, oracle_project

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_edge_ref.npz"))
META = json.loads(bytes(G["meta"]).decode())


def shader_outputs(name):
    return rec.unpack(G["vs_" + name])


@pytest.fixture(scope="module")
def cases():
    return {name: rec.make_case(name) for name in rec.CASES}


@pytest.fixture(scope="module")
def drawn(cases):
    return {name: shader_verdicts(shader_outputs(name))[0] for name in rec.CASES}


# ------------------------------------------------------------------------------------------------ the case list itself
def test_case_sizes_and_the_golden_files_size(cases):
    total = 0
    for name, case in cases.items():
        n = case["centers"].shape[0]
        assert n <= 2000 and n % 256 != 0 and G["vs_" + name].shape == (n, 16), name
        assert tuple(case["uniforms"]["viewport"]) == (512, 288) and np.array_equal(np.asarray(case["uniforms"]["model_view"]), np.eye(4).reshape(16))
        covered = np.concatenate([g["idx"] for g in case["groups"].values()])
        assert np.array_equal(np.sort(covered), np.arange(n)), name                      # every splat belongs to one group
        total += n
    assert total <= 12000, total
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.getsize(os.path.join(here, "golden", "raster_edge_ref.npz")) < os.path.getsize(os.path.join(here, "golden", "raster_ref.npz"))
    assert not any("vert" in f or "frag" in f for f in G.files)


def test_recorded_shader_builds(cases):
    old = json.loads(bytes(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_ref.npz"))["meta"]).decode())
    builds = rec.shader_builds()
    assert set(META["builds"]) == {case["build"] for case in cases.values()}
    for name, m in META["builds"].items():                    # the texts raster_ref.npz was made from
        assert m["vert_sha256"] == old[name]["vert_sha256"] and m["frag_sha256"] == old[name]["frag_sha256"], name
    for name, case in cases.items():
        b = builds[case["build"]]
        assert (case["dynamic"], case["effects"], case["antialiased"]) == (b["dynamicMode"], b["enableOptionalEffects"], b["antialiased"])
        assert (case["kernel2d"], case["max_splat_px"]) == (b["kernel2DSize"], b["maxScreenSpaceSplatSize"]), name
        assert case["sh_stored"] == b["maxSphericalHarmonicsDegree"], name


# ------------------------------------------------------------------------------------------------ census
def stepped_values(case, ladder):
    """The one input that changes along a ladder, float32 per rung: a centre component, a covariance entry or the scene's opacity."""
    if case["effects"] and len(set(case["scene_idx"][ladder].tolist())) == len(ladder):
        return np.asarray(case["uniforms"]["scene_opacity"], np.float32)[case["scene_idx"][ladder]]
    table = np.concatenate([case["centers"][ladder], case["scene"].cov[ladder]], axis=1)
    moving = np.flatnonzero((table != table[0]).any(axis=0))
    assert len(moving) == 1, moving
    return table[:, moving[0]]


def test_census_is_recorded_and_holds(cases):
    assert set(META["census"]) == set(rec.CASES)
    knife_by_camera = {"perspective": 0, "orthographic": 0}
    ladders = exact = 0
    for name in rec.CASES:
        case, c = cases[name], META["census"][name]
        assert c == edge_census(case, shader_outputs(name)), name                        # recounted from the stored outputs
        assert c["least_reach_px"] >= 2.0 and c["least_half_extent_px"] >= 1.0, (name, c["least_reach_px"], c["least_half_extent_px"])
        assert c["drawn"] > 100, name
        for group, g in c["groups"].items():
            where = (name, group, g)
            assert g["drawn"] + g["rejected"] + g["early"] <= g["count"]
            if g["kind"] == "knife":
                assert g["drawn"] >= 0.25 * g["count"] and g["early"] >= 0.25 * g["count"] and g["drawn"] + g["early"] == g["count"], where
                knife_by_camera["orthographic" if case["uniforms"]["orthographic"] else "perspective"] += g["count"]
            elif g["kind"] == "always":
                assert g["drawn"] == g["count"], where
            elif g["kind"] == "never":
                assert g["drawn"] == 0, where
            for verdicts, ladder in zip(g["ladders"], case["groups"][group]["ladders"]):
                changes = [k for k in range(len(verdicts) - 1) if verdicts[k] != verdicts[k + 1]]
                assert len(changes) == 1, where
                ladders += 1
                if case["groups"][group]["exact"]:
                    values = stepped_values(case, ladder)
                    k = changes[0]
                    gap = int(np.abs(values[k + 1]).view(np.uint32)) - int(np.abs(values[k]).view(np.uint32))
                    assert gap == 1 and values[k + 1] != values[k], (where, k, gap)      # between two adjacent floats
                    assert (np.diff(np.abs(values).astype(np.float64)) > 0).all(), where
                    exact += 1
            assert (g["kind"] == "ladder") == bool(g["ladders"]), where
            if case["groups"][group]["observe"] != "drawn":     # continuous at the threshold: every rung is drawn
                assert g["drawn"] == g["count"], where
    assert min(knife_by_camera.values()) >= 600, knife_by_camera
    for name in rec.KNIFE_CASES:
        assert any(g["kind"] == "knife" for g in META["census"][name]["groups"].values()), name
    print(f"{ladders} ladders, {exact} of adjacent floats; knife-edge splats per camera kind {knife_by_camera}")
    # planes (perspective, orthographic), depths, opacity, eigenValue2, alpha; the size cap and the fade (continuous: nothing is decided)
    assert ladders == 32 + 12 + 4 + 12 + 6 + 3 + 6 + 4 and exact == ladders


def test_drawn_knife_edge_splats_are_drawn_tall(cases, drawn):
    """a > d, and basisVector1 - the LONG one - lies along y: eigenVector1 = (0, +-1)."""
    for name in rec.KNIFE_CASES:
        case, res = cases[name], shader_outputs(name).astype(np.float64)
        b1 = res[:, 2, 0:2] - res[:, 1, 0:2]
        b2 = res[:, 1, 0:2] - res[:, 0, 0:2]
        for group, g in case["groups"].items():
            if g["kind"] == "knife":
                k = g["idx"][drawn[name][g["idx"]]]
                assert (b1[k, 0] == 0).all() and (b2[k, 1] == 0).all() and (np.abs(b1[k, 1]) * 288 > np.abs(b2[k, 0]) * 512).all(), (name, group)


def test_clip_block_hugs_the_plane_with_whole_storage_blocks(cases, drawn):
    """Upload order is storage order for this case: block 0 is 256 splats at ONE depth, each 0 to 8 floats inside x = 1.2 w (nine floats
    further out the plane test rejects every one), so the box k_block_test sees is a sliver whose corners sit AT the plane."""
    case = cases["clip_block"]
    assert case["keep_order"] and drawn["clip_block"].all() and len(drawn["clip_block"]) == 300
    c = case["centers"]
    assert len(set(c[:256, 2].tolist())) == 1 and len(set(c[256:, 2].tolist())) == 1
    for block in (slice(0, 256), slice(256, 300)):
        x = c[block, 0]
        assert int(x.view(np.uint32).max()) - int(x.view(np.uint32).min()) == 8
    out = c.copy()
    out[:, 0] = (c[:, 0].view(np.uint32) + np.uint32(9)).view(np.float32)
    assert not raster_edge_ref.verdicts(case, centers=out)[0].any()


# ------------------------------------------------------------------------------------------------ the C oracle
@pytest.mark.parametrize("name", rec.CASES)
def test_c_oracle_gives_the_shaders_verdict_on_every_splat(cases, drawn, name):
    case = cases[name]
    o = oracle_project(case, _oracle_camera(case))
    wrong = np.flatnonzero((o["visible"] == 1) != drawn[name])
    assert len(wrong) == 0, (name, wrong[:10].tolist())
    worst = check_oracle_projection(case, shader_outputs(name), o)
    print(f"{name}: {int(drawn[name].sum())} drawn; worst centre {worst['centre']:.2e} px, basis {worst['basis']:.3f} of its gate, "
          f"colour {worst['colour']:.2e}")


def test_c_oracle_caps_and_fades_at_the_shaders_floats(cases):
    """The size cap and the fade are continuous at their thresholds, so no verdict depends on them; the ladders still pin the float at
    which each sets in.  Fade: vColor.a is the splat's own alpha up to visibleRegionFadeStartRadius and 0 from 0.75 behind it, in the
    shader's outputs and in the C oracle's at the same rungs.  Cap: the oracle's basisVector1 stops growing at the rung the restatement
    names, and from there on the shader's quad is the last rung's (below it the quad may already round to the same floats)."""
    case = cases["fade_ladders"]
    o, res = oracle_project(case, _oracle_camera(case)), shader_outputs("fade_ladders")
    for group, want in (("fade_start", case["rgba"][:, 3].astype(np.float32) * (np.float32(1.0) / np.float32(255.0))), ("fade_end", np.zeros(len(o["a"]), np.float32))):
        for ladder in case["groups"][group]["ladders"]:
            seen = rec.observed(case, res, group, ladder)
            assert np.array_equal(o["a"][ladder] == want[ladder], seen) and seen.any() and not seen.all(), (group, seen)
    for name in ("cap_1024", "cap_48"):
        case = cases[name]
        o, res = oracle_project(case, _oracle_camera(case)), shader_outputs(name)
        capped = raster_edge_ref.verdicts(case, capped=True)[0]
        for ladder in case["groups"]["cap"]["ladders"]:
            assert "".join("1" if v else "0" for v in capped[ladder]) == "0000011111", name
            at_cap = o["b1y"][ladder] == np.float32(case["max_splat_px"])               # (the last rungs below may round to the cap)
            assert at_cap[capped[ladder]].all() and not at_cap[:2].any() and (np.diff(o["b1y"][ladder]) >= 0).all(), name
            assert rec.observed(case, res, "cap", ladder)[capped[ladder]].all(), name


# ------------------------------------------------------------------------------------------------ the restatement and its mutations
@pytest.mark.parametrize("name", rec.CASES)
def test_restatement_gives_the_shaders_verdict_on_every_splat(cases, drawn, name):
    got, stages = raster_edge_ref.verdicts(cases[name])
    wrong = np.flatnonzero(got != drawn[name])
    assert len(wrong) == 0, (name, wrong[:10].tolist())
    _, reject, _ = shader_verdicts(shader_outputs(name))
    assert np.array_equal(stages["scene"] | stages["plane"], reject), name               # gl_Position = (0, 0, 2, 1): exactly these two


PLANE_GROUPS = {(c, p) for c in ("planes_persp", "planes_ortho") for p in rec.PLANES}
KNIFE_GROUPS = {("knife_persp", "knife_axis"), ("knife_persp", "knife_row"), ("knife_persp", "knife_column"), ("knife_ortho", "knife_any"),
                ("knife_ortho_half", "knife_any"), ("knife_aa_scale", "knife_axis"), ("knife_aa_scale", "knife_row"),
                ("knife_aa_scale", "knife_column"), ("knife_dynamic", "knife_axis"), ("knife_dynamic", "knife_row"),
                ("knife_dynamic", "knife_column")}
# (mutation, the groups in which it MUST change a verdict, may it change verdicts elsewhere?)
MUTATIONS = {
    "x_hi_swapped": (dict(swap={"x_hi"}), {("planes_persp", "x_hi"), ("planes_ortho", "x_hi"), ("clip_block", "hugging")}, False),
    "x_lo_swapped": (dict(swap={"x_lo"}), {("planes_persp", "x_lo"), ("planes_ortho", "x_lo")}, False),
    "y_hi_swapped": (dict(swap={"y_hi"}), {("planes_persp", "y_hi"), ("planes_ortho", "y_hi")}, False),
    "y_lo_swapped": (dict(swap={"y_lo"}), {("planes_persp", "y_lo"), ("planes_ortho", "y_lo")}, False),
    "z_near_swapped": (dict(swap={"z_near"}), {("planes_ortho", "z_near")}, True),
    "z_far_swapped": (dict(swap={"z_far"}), {("planes_persp", "z_far"), ("planes_ortho", "z_far")}, False),
    "opacity_swapped": (dict(swap={"opacity"}), {("scene_ladders", "opacity")}, False),
    "aa_swapped": (dict(swap={"aa"}), {("arith_aa", "aa_ratio_one")}, True),
    "eig2_swapped": (dict(swap={"eig2"}), {("arith_ortho", "eig2")}, True),
    "1.2_up": (dict(ulp={"1.2": 1}), PLANE_GROUPS, False),
    "1.2_down": (dict(ulp={"1.2": -1}), PLANE_GROUPS | {("clip_block", "hugging")}, False),
    "0.1_up": (dict(ulp={"0.1": 1}), {("arith_ortho", "floor")}, True),
    "0.01_up": (dict(ulp={"0.01": 1}), {("scene_ladders", "opacity")}, False),
    "0.01_down": (dict(ulp={"0.01": -1}), {("scene_ladders", "opacity")}, False),
    "fused_discriminant": (dict(fused_disc=True), KNIFE_GROUPS, True),
    "split_trace": (dict(split_trace=True), {("arith_ortho", "overflow")}, False),
    "no_nan_check": (dict(no_nan_check=True), KNIFE_GROUPS | {("arith_ortho", "overflow"), ("degenerate", "covariance")}, True),
    "no_z_test": (dict(no_z_test=True), {(c, z) for c in ("planes_persp", "planes_ortho") for z in ("z_near", "z_far")}, False),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_mutated_restatement_changes_a_verdict_in_its_class(cases, drawn, mutation):
    mut, must, elsewhere = MUTATIONS[mutation]
    changed = {}
    for name, case in cases.items():
        differ = raster_edge_ref.verdicts(case, mut)[0] != drawn[name]
        for group, g in case["groups"].items():
            if differ[g["idx"]].any():
                changed[(name, group)] = int(differ[g["idx"]].sum())
    print(mutation, changed)
    assert must <= set(changed), (mutation, "no verdict changes in", sorted(must - set(changed)))
    if not elsewhere:
        assert set(changed) == must, (mutation, sorted(set(changed) - must))


def test_the_floor_one_ulp_down_is_not_observable():
    """max(0.1, x) feeds a sqrt alone, and sqrt maps the float below 0.1f to the float 0.1f maps to: no mutation is asked for it."""
    below = np.nextafter(np.float32(0.1), np.float32(0.0))
    assert np.sqrt(below) == np.sqrt(np.float32(0.1)) != np.sqrt(np.nextafter(np.float32(0.1), np.float32(1.0)))
