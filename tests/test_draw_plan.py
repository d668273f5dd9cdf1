"""The host policy of a draw (csrc/draw_plan.cpp) held to its host model (draw_plan_ref.py) through the library's pure-host debug
entry: no GPU.  The policy decides where the block test runs, the size of the list bins, whether the previous draw's statistics
order the blend's bins and shifted by how much, whether the deep pass runs and where its workgroups sit - nothing a frame test
can see.  The cases (draw_plan_cases.py) are chosen so that fp32 and fp64 cannot decide them differently; the model checks that
itself and refuses a case that is not."""
import ctypes as C
import math

import pytest

import draw_plan_cases as dc
import draw_plan_ref as ref
import gaussiansplats3d_amd as g

CASES = dc.cases()


def _entry():
    fn = g.load().gs_debug_draw_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(dc.PlanIn), C.POINTER(dc.PlanOut)]
    return fn


def library(inputs):
    s, out = dc.to_struct(inputs), dc.PlanOut()
    assert _entry()(C.byref(s), C.byref(out)) == 0
    return {name: getattr(out, name) for name in dc.FIELDS_OUT}


def test_every_case_is_one_fp32_and_fp64_decide_alike():
    assert len(CASES) == len(set(name for name, _, _ in CASES))
    for name, inputs, _ in CASES:
        ref.draw_plan(inputs)                              # raises on a borderline case: none may be left out


@pytest.mark.parametrize("name,inputs,expect", CASES, ids=[c[0] for c in CASES])
def test_library_decides_as_the_model(name, inputs, expect):
    want = ref.draw_plan(inputs)
    got = library(inputs)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    expect = dict(expect)
    turn = expect.pop("turn", None)
    if turn is not None:                                   # turning in place: the shift is the turn, to the nearest bin (1.5 -> 2)
        for s, bins in ((got["sx"], turn[0]), (got["sy"], -turn[1])):
            assert s == math.copysign(math.floor(abs(bins) + 0.5), bins), (got["sx"], got["sy"], turn)
    for key, value in expect.items():                      # what the case is there to show
        assert got[key] == value, (key, got[key], value)


def test_null_arguments_are_refused():
    assert _entry()(None, None) == -1


def test_list_shift_hysteresis_walk():
    """A ratio of tiles per visible splat walking up and down across every threshold takes the model's level sequence."""
    got, want = [3], [3]
    for ratio in dc.HYSTERESIS_WALK:
        tiles16 = int(ratio * dc.HYSTERESIS_VISIBLE)
        got.append(library(dc.make_inputs(list_current=got[-1], tiles16=tiles16, visible=dc.HYSTERESIS_VISIBLE))["list_shift"])
        want.append(ref.adapt_list_shift(want[-1], tiles16, dc.HYSTERESIS_VISIBLE))
    assert got == want
    assert set(want) == {1, 3, 4, 5}                       # every level was reached ...
    ups = sum(b > a for a, b in zip(want, want[1:]))
    downs = sum(b < a for a, b in zip(want, want[1:]))
    assert ups >= 4 and downs >= 4                         # ... from both sides
    # inside a hysteresis band the size stays where it was, whichever side it came from
    for level, ratio in ((1, 3.1), (3, 3.1), (3, 20.0), (4, 20.0), (4, 79.0), (5, 79.0)):
        assert library(dc.make_inputs(list_current=level, tiles16=int(ratio * 1000), visible=1000))["list_shift"] == level
    assert library(dc.make_inputs(list_current=4, tiles16=123456, visible=0))["list_shift"] == 4       # nothing visible: unchanged


def test_the_model_refuses_borderline_inputs():
    with pytest.raises(AssertionError):
        ref.adapt_list_shift(3, 324 * 1000, 100 * 1000)    # on the threshold 3.24
    with pytest.raises(AssertionError):
        ref.block_test_mode(90, 100, 0, 1, 0, 0)           # a share of 0.9
    with pytest.raises(AssertionError):
        ref.plan_schedule(dc.make_inputs(now=dc.cam_turned(1.5, 0), centre_sum=dc.centre_sum(dc.LOOK)))   # a shift of 1.5 bins
