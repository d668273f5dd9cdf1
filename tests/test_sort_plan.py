"""The host policy of a depth sort (csrc/sort_plan.cpp) held to its host model (sort_plan_ref.py, written from the sorter as it was
before the plan existed) through the library's pure-host debug entry: no GPU.  The plan decides what becomes of a pending gather,
which front end keys the list and on which grids, pass 0's slot of group rows, and what every radix pass reads and writes - a
wrong decision is a wrong list or a store through offsets nobody wrote, which a sort test sees only for the sizes it happens to run."""
import ctypes as C

import pytest

import gaussiansplats3d_amd as g
import sort_plan_cases as sc
import sort_plan_ref as ref

CASES = sc.cases()


def _entry():
    fn = g.load().gs_debug_sort_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(sc.PlanIn), C.POINTER(sc.PlanOut)]
    return fn


def library(inputs):
    s, out = sc.to_struct(inputs), sc.PlanOut()
    assert _entry()(C.byref(s), C.byref(out)) == 0
    return sc.out_from_struct(out)


differences = sc.differences


def test_case_names_are_unique_and_the_structs_are_words():
    assert len(CASES) == len(set(name for name, _, _ in CASES))
    assert C.sizeof(sc.PlanIn) == 4 * (len(sc.IN_WORDS) + 2 + len(sc.SWITCHES))
    assert C.sizeof(sc.PlanOut) == 4 * (len(ref.PLAN_FIELDS) + ref.RADIX_MAX_PASSES * len(ref.PASS_FIELDS))


@pytest.mark.parametrize("name,inputs,check", CASES, ids=[c[0] for c in CASES])
def test_library_decides_as_the_model(name, inputs, check):
    want = ref.sort_plan(inputs)
    got = library(inputs)
    assert not differences(got, want), differences(got, want)
    check(got)                                             # what the case is there to show


def test_null_arguments_are_refused():
    assert _entry()(None, None) == -1


def test_clean_slot_alternates_over_a_sequence_of_plans():
    slot = 3                                               # a new sorter's
    for k, (kw, pass0_slot, after) in enumerate(sc.clean_slot_sequence()):
        inputs = sc.make_inputs(clean_slot=slot, **kw)
        got = library(inputs)
        assert not differences(got, ref.sort_plan(inputs))
        assert (got["pass0_slot"], got["next_clean_slot"]) == (pass0_slot, after), (k, got["pass0_slot"], got["next_clean_slot"])
        if got["passes"]:
            assert {got["pass0_slot"], got["next_clean_slot"]} == {0, 3}
            assert [p["slot"] for p in got["pass"][1:got["passes"]]] == list(range(1, got["passes"]))
        slot = got["next_clean_slot"]


def test_grids_against_their_tables():
    """The two grid functions over every length at which either changes its mind, and around them."""
    marks = {0, 1, ref.RADIX_TILE, 512 * ref.RADIX_TILE, 1024 * ref.RADIX_TILE, 1536 * ref.RADIX_TILE, 2048 * 3 * ref.RADIX_TILE, (1 << 32) - ref.RADIX_TILE}
    for m in sorted(marks):
        for n in range(max(m - 2, 0), min(m + 3, 1 << 32)):
            got = library(sc.make_inputs(n=n, precision=10, extreme_current=0))
            if n == 0:
                assert got["passes"] == 0
                continue
            chunk = ref.radix_chunk_grid_for(n) if got["val_bits"] <= 24 else 0     # (a 25-bit payload rules the kernel out by itself)
            assert got["pass"][0]["chunked"] == (1 if chunk else 0), n
            assert got["pass"][0]["grid"] == (chunk if chunk else ref.radix_grid_for(n)), n
            assert 1 <= got["pass"][0]["grid"] <= (ref.RADIX_MAX_BLOCKS if chunk else ref.RADIX_TILE_GRID), n
