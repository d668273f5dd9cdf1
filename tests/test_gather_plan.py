"""The host policy of an octree gather and its hand-over to a sorter (csrc/gather_plan.cpp) held to their host models
(gather_plan_ref.py) through the library's pure-host debug entries: no GPU.

The plan: the cull thresholds and the bucket scale reach the kernels as arguments and decide, bit for bit, which leaves are culled
and how they spread - the library's doubles must equal the model's as bit patterns (both are IEEE doubles rounded once per
operation: a difference is a finding, not a tolerance).  The hand-over: after every event of every script the library's record
of each sorter, each tree's back-pointer and the action it asks of the caller equal the three-state model's."""
import ctypes as C

import pytest

import gather_plan_cases as gc
import gather_plan_ref as ref
import gaussiansplats3d_amd as g

PLAN_CASES = gc.plan_cases()
SCRIPTS = gc.handover_scripts()


def _plan_entry():
    fn = g.load().gs_debug_gather_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(gc.PlanIn), C.POINTER(gc.PlanOut)]
    return fn


def library_plan(inputs):
    s, out = gc.to_struct(inputs), gc.PlanOut()
    assert _plan_entry()(C.byref(s), C.byref(out)) == 0
    return {n: getattr(out, n) for n in gc.OUT_DOUBLES + gc.OUT_WORDS}


def as_bits(plan):
    return {k: gc.bits(v) if k in gc.OUT_DOUBLES else v for k, v in plan.items()}


@pytest.mark.parametrize("name,inputs,expect", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_library_plans_as_the_model_bit_for_bit(name, inputs, expect):
    want, got = ref.gather_plan(inputs), library_plan(inputs)
    assert as_bits(got) == as_bits(want), {k: (got[k], want[k]) for k in got if as_bits(got)[k] != as_bits(want)[k]}
    assert ref.buckets_in_range(inputs, want["scale"])      # no corner of a scene box falls beyond the last bucket
    for key, value in expect.items():                       # what the case is there to show
        assert got[key] == value, (key, got[key], value)


def test_the_cases_cover_what_they_name():
    names = [c[0] for c in PLAN_CASES]
    assert len(names) == len(set(names)) and sum(n.startswith("kat_") for n in names) == 21
    scales = {gc.bits(ref.gather_plan(i)["scale"]) for _, i, _ in PLAN_CASES}
    assert len(scales) > 20                                 # the cameras do spread the scale
    by_name = {n: i for n, i, _ in PLAN_CASES}
    d = ref.corner_distances(by_name["corner_with_zero_w"]["scenes"][0])
    assert all(map(lambda v: v == v and v != float("inf"), d)) and ref.gather_plan(by_name["corner_with_zero_w"])["scale"] != 1.0
    assert all(v == 0.0 for v in ref.corner_distances(by_name["box_collapsed_to_the_eye"]["scenes"][0]))
    wide, narrow = by_name["demo_garden_7680"], by_name["demo_garden_1920"]      # same aspect, same fov: the same thresholds
    assert ref.thresholds(50.0, 7680.0, 4320.0) == ref.thresholds(50.0, 1920.0, 1080.0) and wide["render_width"] != narrow["render_width"]


def test_policy_over_the_full_cross_product():
    seen = set()
    for k, inputs in gc.policy_inputs():
        want, got = ref.gather_plan(inputs), library_plan(inputs)
        assert as_bits(got) == as_bits(want), (k, got, want)
        # said once more, from the rule: only a static sorter that is the list's only reader defers the copy of a plain tree
        deferred = k["has_sorter"] and not (k["dynamic"] or k["host_copy"] or k["no_defer"] or k["several_scenes"] or k["no_leaves"])
        assert got["deferred"] == int(bool(deferred)) and got["zero_keep"] == int(bool(deferred and k["frustum_cull"]))
        assert got["keep_words"] == ((40001 + 63) // 64 + 2 if got["zero_keep"] else 0)
        assert got["keep_words"] * 8 <= ((50000 + 63) // 64 + 8) * 8      # ... inside the sorter's keep mask
        assert got["leaf_grid"] == (0 if k["no_leaves"] else 102) and got["scene_table"] == k["several_scenes"]
        seen.add((got["deferred"], got["zero_keep"], got["scene_table"], got["leaf_grid"] != 0))
    assert len(seen) == 2 * 2 + 1 + 1                        # (not deferred) x scene table x leaves, deferred, deferred + zeroed mask


def test_plan_null_arguments_are_refused():
    assert _plan_entry()(None, None) == -1


# ------------------------------------------------------------------------------------------------------------------ hand-over
def library_replay(events):
    fn = g.load().gs_debug_gather_handover
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(gc.Event), C.c_uint32, C.POINTER(gc.Step)]
    ev = (gc.Event * max(len(events), 1))()
    for k, e in enumerate(events):
        for n in ("kind", "tree", "sorter", "a", "b", "c", "d"):
            setattr(ev[k], n, e.get(n, 0))
    steps = (gc.Step * max(len(events), 1))()
    assert fn(ev, len(events), steps) == 0
    return [dict({n: list(getattr(s, n)) for n in gc.STEP_PAIRS}, **{n: getattr(s, n) for n in gc.STEP_WORDS}) for s in steps[:len(events)]]


def model_replay(events):
    m = ref.Handover()
    return [m.step(**e) for e in events]


def check_invariant(step):
    """A tree's back-pointer names a sorter exactly when that sorter is PLANNED on that tree."""
    for t in (0, 1):
        for s in (0, 1):
            assert (step["planner"][t] == s) == (step["state"][s] == ref.PLANNED and step["tree_of"][s] == t), step
    for s in (0, 1):
        assert step["state"][s] == ref.PLANNED or (step["tree_of"][s] == ref.NOBODY and not step["keep_zeroed"][s]), step


@pytest.mark.parametrize("name,events,expect", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_library_hands_over_as_the_model(name, events, expect):
    got, want = library_replay(events), model_replay(events)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, events[k], {f: (a[f], b[f]) for f in a if a[f] != b[f]})
        check_invariant(a)
    for k, fields in expect.items():                         # what the script is there to show
        for f, v in fields.items():
            assert got[k][f] == v, (k, f, got[k][f], v)


def test_random_walk_of_events():
    events = gc.random_walk(20240611, 4000)
    got, want = library_replay(events), model_replay(events)
    states = set()
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, events[k], {f: (a[f], b[f]) for f in a if a[f] != b[f]})
        check_invariant(a)
        states.add((tuple(a["state"]), tuple(a["planner"])))
    assert {s for s, _ in states} == {(x, y) for x in range(3) for y in range(3)}      # every pair of states was reached ...
    assert ((ref.PLANNED, ref.PLANNED), (1, 0)) in states and ((ref.PLANNED, ref.PLANNED), (0, 1)) in states     # ... on either tree
    assert sum(a["evicted"] != ref.NOBODY for a in got) > 50 and {a["refused"] for a in got} == {0, 1, 2}


def test_replay_refuses_bad_scripts():
    fn = g.load().gs_debug_gather_handover
    fn.restype = C.c_int
    assert fn(None, 0, None) == -1
    for bad in (dict(kind=7), dict(kind=0, tree=2), dict(kind=1, sorter=2), dict(kind=0, sorter=3)):
        ev, st = (gc.Event * 1)(), (gc.Step * 1)()
        for n, v in bad.items():
            setattr(ev[0], n, v)
        assert fn(ev, 1, st) == -1, bad
