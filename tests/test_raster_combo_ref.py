"""CPU tier of the COMBINED shader permutations.  tests/golden/raster_combo_ref.npz holds what the reference's own GLSL computes for
the cases of tests/raster_combo_cases.py, in which several features are on together (oracle/make_golden_raster.py --combos); the
C raster oracle's vertex stage is held to it with the gate of test_raster_ref.py, tolerances unchanged.

Three things keep the list honest:
  * the census: counts taken from the shader's outputs while the golden was made (every scene draws, every fade band and every
    reject rule is populated), recorded in the file and asserted here;
  * mutations: a wrong per-scene input given to the oracle's camera alone must break the gate on the cases named for it;
  * the recorded material state of the new shader builds.
The observed worst differences are printed per case, as the record the first device run compares with."""
import json
import os

import numpy as np
import pytest

import oracle
import raster_combo_cases as rcc
from oracle.make_golden_raster import combo_census
from test_raster_ref import _from_shader, _oracle_camera, check_oracle_projection, oracle_project

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_combo_ref.npz"))
META = json.loads(bytes(G["meta"]).decode())


@pytest.fixture(scope="module")
def cases():
    return {name: rcc.make_case(name) for name in rcc.CASES}


@pytest.mark.parametrize("name", rcc.CASES)
def test_c_oracle_vertex_stage_matches_the_reference_shader_on_combined_permutations(cases, name):
    case = cases[name]
    worst = check_oracle_projection(case, G["vs_" + name], oracle_project(case, _oracle_camera(case)))
    print(f"{name}: worst centre {worst['centre']:.2e} px (gate 2e-3), basis {worst['basis']:.3f} of its gate, "
          f"colour {worst['colour']:.2e} (gate {2e-4 if case['dynamic'] else 3e-6:.0e})")


# ------------------------------------------------------------------------------------------------ mutations
def _same_range(case, ocam):
    for s_ in range(rcc.GS_MAX_SCENES):
        ocam.sh8_min[s_], ocam.sh8_max[s_] = ocam.sh8_min[0], ocam.sh8_max[0]


def _world_camera_position(case, ocam):
    for s_ in range(rcc.GS_MAX_SCENES):
        ocam.inv_cam_pos[s_][:] = list(ocam.cam_pos)


def _opaque(case, ocam):
    for s_ in range(rcc.GS_MAX_SCENES):
        ocam.opacity[s_] = 1.0


def _all_visible(case, ocam):
    for s_ in range(rcc.GS_MAX_SCENES):
        ocam.visible[s_] = 1


def _moved_fade_centre(case, ocam):
    t = np.asarray(case["uniforms"]["transforms"][0], np.float64)[12:15]          # the first scene's translation
    assert np.linalg.norm(t) > 0.1
    ocam.scene_center[:] = (np.asarray(case["uniforms"]["scene_center"], np.float64) + t).astype(np.float32).tolist()


MUTATIONS = [(_same_range, "scenes_sh8"), (_same_range, "dyn_fx_aa_sh8_fade"), (_same_range, "dyn_fx_32_scenes"),
             (_world_camera_position, "dyn_fx_aa_sh8_fade"), (_world_camera_position, "dyn_ortho_aa"),
             (_opaque, "dyn_fx_aa_sh8_fade"), (_opaque, "dyn_fx_32_scenes"),
             (_all_visible, "dyn_fx_aa_sh8_fade"),
             (_moved_fade_centre, "dyn_fx_aa_sh8_fade"),
             ("rolled_scene_indexes", "dyn_fx_32_scenes")]


@pytest.mark.parametrize("mutate,name", MUTATIONS, ids=lambda v: v if isinstance(v, str) else v.__name__.strip("_"))
def test_a_wrong_per_scene_input_breaks_the_gate(cases, mutate, name):
    case = cases[name]
    ocam = _oracle_camera(case)
    scene_idx = None
    if mutate == "rolled_scene_indexes":
        scene_idx = np.roll(case["scene_idx"], 1)
    else:
        mutate(case, ocam)
    with pytest.raises(AssertionError) as failure:
        check_oracle_projection(case, G["vs_" + name], oracle_project(case, ocam, scene_idx))
    if mutate is _all_visible:                                # the invisible scene is drawn: decisions, not values
        assert "accept / reject decisions" in str(failure.value)


# ------------------------------------------------------------------------------------------------ census, recorded state
def test_every_case_is_populated_by_the_reference_shader_alone(cases):
    assert set(META["census"]) == set(rcc.CASES)
    for name in rcc.CASES:
        case, c = cases[name], META["census"][name]
        # what is recorded is the stored outputs' own count (all but the antialiased-only rejects, which need the sibling build's run)
        assert {k: v for k, v in c.items() if k != "aa_only_rejects"} == combo_census(case, G["vs_" + name], None), name
        assert c["drawn"] == int(_from_shader(G["vs_" + name], case["uniforms"]["viewport"])[0].sum()) >= 300, name
        gone = rcc.scene_rejected(case)
        for s_, (d, r) in enumerate(zip(c["drawn_per_scene"], c["rejected_per_scene"])):
            assert (d == 0 and r >= 50) if gone[s_] else d >= 10, (name, s_, d, r)
        assert ("fade_partial" in c) == (name in rcc.FADE_CASES), name
        if name in rcc.FADE_CASES:
            assert c["fade_partial"] >= 50 and c["fade_zero"] >= 50, (name, c)
        assert ("aa_only_rejects" in c) == (name in rcc.AA_REJECT_CASES), name
        if name in rcc.AA_REJECT_CASES:
            assert c["aa_only_rejects"] >= 10, (name, c)
    assert sum(rcc.scene_rejected(cases["dyn_fx_aa_sh8_fade"])) == 2
    assert META["census"]["dyn_fx_clamp"]["at_clamp"] >= 20
    assert cases["dyn_fx_32_scenes"]["uniforms"]["scene_count"] == rcc.GS_MAX_SCENES == int(cases["dyn_fx_32_scenes"]["scene_idx"].max()) + 1
    for name in ("scenes_sh8", "dyn_fx_aa_sh8_fade", "dyn_fx_clamp", "fx_aa_fade_eval1", "dyn_fx_32_scenes"):   # a range per scene
        r = cases[name]["uniforms"]["sh8_range"]
        assert cases[name]["sh8"] and len(set(r)) == len(r) == cases[name]["uniforms"]["scene_count"], name


def test_recorded_combined_shader_builds_and_blend_state(cases):
    builds = rcc.shader_builds()
    assert set(META["builds"]) == set(builds) and set(META["census_builds"]) == set(rcc.census_builds())
    for m in list(META["builds"].values()) + list(META["census_builds"].values()):   # SplatMaterial3D.js:65-75
        assert m["state"]["blending"] == 1 and m["state"]["transparent"] and m["state"]["depthTest"] and not m["state"]["depthWrite"]
        assert len(m["vert_sha256"]) == 64 and len(m["frag_sha256"]) == 64
    # the three reused builds are the texts raster_ref.npz was made from; every build's text is its own
    old = json.loads(bytes(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_ref.npz"))["meta"]).decode())
    for name in ("base2", "dynamic2", "effects1"):
        assert META["builds"][name]["vert_sha256"] == old[name]["vert_sha256"], name
    texts = [m["vert_sha256"] for m in META["builds"].values()] + [m["vert_sha256"] for m in META["census_builds"].values()]
    assert len(set(texts)) == len(texts)
    for name, b in builds.items():                            # the per-scene uniforms a build declares follow its switches
        un = META["builds"][name]["state"]["uniforms"]
        assert ("transforms" in un) == b["dynamicMode"] and ("sceneOpacity" in un) == b["enableOptionalEffects"], name
    for name, case in cases.items():                          # and every case's switches are its build's
        b = builds[case["build"]]
        assert (case["dynamic"], case["effects"], case["antialiased"]) == (b["dynamicMode"], b["enableOptionalEffects"], b["antialiased"])
        assert (case["kernel2d"], case["max_splat_px"]) == (b["kernel2DSize"], b["maxScreenSpaceSplatSize"]), name
        assert case["sh_stored"] == b["maxSphericalHarmonicsDegree"], name
    assert "vs_" + rcc.CASES[0] in G.files and not any("vert" in f or "frag" in f for f in G.files)
