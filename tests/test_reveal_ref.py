"""CPU tier: the host model of gs_mesh_bounds (bounds_ref) and the two statements of the scene-reveal state machine
(gaussiansplats3d_amd/reveal.py, node/VisibleRegion.mjs) against what the reference itself computed (tests/golden/reveal_kat.json,
recorded by tests/tools/make_reveal_golden.py) - bit for bit: doubles are compared with ==."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounds_ref
import reveal_cases as cases
from gaussiansplats3d_amd import reveal
from gaussiansplats3d_amd.reveal import SceneRevealMode, VisibleRegion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bounds_case(c):
    """(centres fp32 [n, 3] in global order, scene index per splat, transforms [scenes, 16])."""
    per_scene = [np.asarray(x, np.float32).reshape(-1, 3) for x in c["centers"]]
    idx = np.concatenate([np.full(len(x), k, np.uint32) for k, x in enumerate(per_scene)])
    return np.concatenate(per_scene), idx, np.asarray(c["transforms"], np.float64)


def test_the_recorded_constants_are_the_modules():
    k = cases.kat()
    assert k["constants"] == {"SCENE_FADEIN_RATE_FAST": reveal.SCENE_FADEIN_RATE_FAST, "SCENE_FADEIN_RATE_GRADUAL": reveal.SCENE_FADEIN_RATE_GRADUAL,
                              "VISIBLE_REGION_EXPANSION_DELTA": reveal.VISIBLE_REGION_EXPANSION_DELTA}
    assert k["modes"] == {"Default": SceneRevealMode.Default, "Gradual": SceneRevealMode.Gradual, "Instant": SceneRevealMode.Instant}
    assert [c["name"] for c in k["bounds"]] == ["identity", "static", "two_scenes"]


@pytest.mark.parametrize("c", cases.kat()["bounds"], ids=lambda c: c["name"])
def test_the_model_reproduces_the_reference_bounds(c):
    centers, idx, transforms = bounds_case(c)
    machine = VisibleRegion()
    machine.update(False, c["sceneCenters"], False,
                   lambda center: math.sqrt(bounds_ref.bounds(centers, center, transforms=transforms, scene_idx=idx)["max_dist_sq"]))
    assert machine.calculated_scene_center == c["calculatedSceneCenter"]
    assert machine.max_splat_distance_from_scene_center == c["maxSplatDistanceFromSceneCenter"]
    plain = bounds_ref.bounds(centers, (0.0, 0.0, 0.0))
    assert plain["min"].tolist() == c["boxPlain"]["min"] and plain["max"].tolist() == c["boxPlain"]["max"]
    moved = bounds_ref.bounds(centers, (0.0, 0.0, 0.0), transforms=transforms, scene_idx=idx)
    assert moved["min"].tolist() == c["boxTransformed"]["min"] and moved["max"].tolist() == c["boxTransformed"]["max"]
    assert plain["count"] == moved["count"] == len(centers)
    # the Float32Array the reference's transformed fill returns = (float) of the model's transformed centres
    baked = np.asarray(c["bakedCenters"], np.float32).reshape(-1, 3)
    assert np.array_equal(bounds_ref.transformed(centers, transforms, idx).astype(np.float32), baked)
    # ... and a mesh that stores THOSE (a baked static transform) is within the derived 2^-24 (R + |center|) of the reference
    R = c["maxSplatDistanceFromSceneCenter"]
    got = math.sqrt(bounds_ref.bounds(baked, c["calculatedSceneCenter"])["max_dist_sq"])
    assert abs(got - R) <= 2.0 ** -24 * (R + float(np.linalg.norm(c["calculatedSceneCenter"])))


def test_the_model_skips_nan_and_keeps_inf():
    c = np.array([[1, 2, 3], [np.nan, 0, 0], [4, -5, 6], [0, np.inf, 0]], np.float32)
    b = bounds_ref.bounds(c, (0, 0, 0), 0, 3)
    assert b["count"] == 2 and b["min"].tolist() == [1, -5, 3] and b["max"].tolist() == [4, 2, 6] and b["max_dist_sq"] == 77.0
    b = bounds_ref.bounds(c, (0, 0, 0))
    assert b["count"] == 3 and b["max"][1] == np.inf and b["max_dist_sq"] == np.inf
    b = bounds_ref.bounds(c, (0, 0, 0), 1, 1)
    assert b["count"] == 0 and b["max_dist_sq"] == 0.0 and not b["min"].any() and not b["max"].any()
    assert bounds_ref.bounds(c, (0, 0, 0), 2, 0)["count"] == 0


@pytest.mark.parametrize("name", cases.script_names())
def test_reveal_py_reproduces_the_reference_states(name):
    s = cases.script(name)
    points = 0
    for where, got, want in cases.replay(s, VisibleRegion(s["multiplier"])):
        assert cases.same(got, want), (where, got, want)
        points += 1
    assert points >= 10


# -- mutations: each wrong version of the machine must leave the recorded states -------------------------------------------------
class FastRateBeforeTheFinalBuild(VisibleRegion):
    def update_fade_distance(self, scene_reveal_mode=SceneRevealMode.Default):
        final, self.final_build = self.final_build, True
        super().update_fade_distance(scene_reveal_mode)
        self.final_build = final


class CompleteAt099(VisibleRegion):
    def update_fade_distance(self, scene_reveal_mode=SceneRevealMode.Default):
        super().update_fade_distance(scene_reveal_mode)
        complete = (self.visible_region_fade_start_radius / self.visible_region_buffer_radius if self.visible_region_buffer_radius > 0 else 0) >= 0.99
        self.shader_fade_in_complete = 1 if (complete or scene_reveal_mode == SceneRevealMode.Instant) else 0
        self.visible_region_changing = not complete


class NoExpansionDelta(VisibleRegion):
    def update(self, since_last_build_only, scene_centers, final_build, max_distance_from):
        def grown(center):
            d = max(max_distance_from(center), self.max_splat_distance_from_scene_center)
            if d > self.visible_region_buffer_radius:         # expand on any growth, not only beyond the delta
                self.visible_region_buffer_radius = d
                self.visible_region_radius = max(d - reveal.VISIBLE_REGION_EXPANSION_DELTA, 0.0)
            return d
        super().update(since_last_build_only, scene_centers, final_build, grown)


class MaximumRestartedOnAnUpdateBuild(VisibleRegion):
    def update(self, since_last_build_only, scene_centers, final_build, max_distance_from):
        if since_last_build_only:
            self.max_splat_distance_from_scene_center = 0.0
        super().update(since_last_build_only, scene_centers, final_build, max_distance_from)


MUTATIONS = {"fast_rate_before_final": (FastRateBeforeTheFinalBuild, "progressive"), "ge_099": (CompleteAt099, "boundary_099"),
             "no_delta_rule": (NoExpansionDelta, "progressive"), "maximum_restarted": (MaximumRestartedOnAnUpdateBuild, "progressive")}


@pytest.mark.parametrize("variant", sorted(MUTATIONS))
def test_a_mutated_machine_leaves_the_recorded_states(variant):
    cls, where = MUTATIONS[variant]
    broken = {}
    for name in cases.script_names():
        s = cases.script(name)
        broken[name] = sum(0 if cases.same(got, want) else 1 for _, got, want in cases.replay(s, cls(s["multiplier"])))
    print(variant, broken)
    assert broken[where] > 0, broken


def test_visible_region_mjs_reproduces_the_reference_states(tmp_path):
    assert shutil.which("node") is not None, "node is part of the toolchain: the Node seam cannot go untested"
    jobs = []
    for name in cases.script_names():
        s = cases.script(name)
        centers = cases.script_centers(s)
        events = []
        for ev in s["events"]:
            if ev["op"] == "build":
                d = cases.range_distance(centers, ev["from"], ev["to"])(ev["calculatedSceneCenter"])
                events.append({"op": "build", "reset": ev["reset"], "update": ev["update"], "finalBuild": ev["finalBuild"], "distance": d})
            else:
                events.append({"op": "frames", "mode": ev["mode"], "count": ev["count"], "keep": [smp[0] for smp in ev["samples"]]})
        jobs.append({"name": name, "multiplier": s["multiplier"], "sceneCenter": s["sceneCenter"], "events": events})
    job = tmp_path / "job.json"
    job.write_text(json.dumps(jobs))
    out = subprocess.check_output(["node", "--no-warnings", os.path.join(ROOT, "tests", "reveal_via_node.mjs"), str(job)], text=True, timeout=120)
    got = json.loads(out.strip().splitlines()[-1])
    points = 0
    for name in cases.script_names():
        s = cases.script(name)
        rows = iter(got[name])
        for e, ev in enumerate(s["events"]):
            if ev["op"] == "build":
                assert cases.same(next(rows), ev["calculatedSceneCenter"] + ev["state"]), (name, e)
                points += 1
            else:
                for smp in ev["samples"]:
                    assert cases.same(next(rows), smp[2:]), (name, e, smp[0])
                    points += 1
    assert points > 500
