"""The host plan of gs_mesh_reorder (csrc/upload_plan.cpp, plan_reorder) held to its bitmap model (reorder_plan_cases.py) through
the library's pure-host debug entry gs_debug_reorder_plan: no GPU.  The plan decides which calls are refused, which do nothing,
which Morton runs the mesh remembers afterwards and which storage blocks get new boxes; gs_mesh_reorder decides nothing else."""
import ctypes as C

import pytest

import gaussiansplats3d_amd as g
import reorder_plan_cases as cases
from reorder_plan_cases import CASES, NOOP, REFUSED, ReorderIn, ReorderOut


def _entry():
    fn = g.load().gs_debug_reorder_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(ReorderIn), C.POINTER(ReorderOut)]
    return fn


def to_struct(state):
    s = ReorderIn()
    for name in ("runs", "slotted"):
        setattr(s, "n_" + name, len(state[name]))
        for k, (a, b) in enumerate(state[name][:cases.DEBUG_MAX]):
            getattr(s, name)[k][0], getattr(s, name)[k][1] = a, b
    s.uploaded, s.reorder, s.from_, s.count = state["uploaded"], state["reorder"], state["from"], state["count"]
    return s


def library(state):
    out = ReorderOut()
    assert _entry()(C.byref(to_struct(state)), C.byref(out)) == 0
    assert not (out.refused and out.noop)
    if out.refused:
        return REFUSED
    if out.noop:
        return NOOP
    return {"runs": [tuple(int(v) for v in out.runs[k]) for k in range(out.n_runs)], "first_block": int(out.first_block),
            "end_block": int(out.end_block)}


def test_the_case_names_are_unique():
    assert len(CASES) == len(set(name for name, _, _ in CASES))


@pytest.mark.parametrize("name,st,expect", CASES, ids=[c[0] for c in CASES])
def test_library_decides_as_the_model(name, st, expect):
    want, got = cases.reorder_plan(st), library(st)
    assert got == want, (got, want)
    if expect in (REFUSED, NOOP):
        assert got == expect
        return
    for key, value in expect.items():                      # what the case is there to show
        assert got[key] == value, (key, got[key], value)
    start, end = st["from"], st["from"] + st["count"]
    assert (start, end) in got["runs"]                     # the range is one run, the others are the runs of before
    assert [r for r in got["runs"] if r != (start, end)] == [r for r in st["runs"] if r[1] <= start or r[0] >= end]
    assert got["first_block"] * cases.BLOCK <= start < (got["first_block"] + 1) * cases.BLOCK
    assert (got["end_block"] - 1) * cases.BLOCK < end <= got["end_block"] * cases.BLOCK


@pytest.mark.parametrize("mutation", cases.MUTATIONS)
def test_the_cases_catch_every_mutation_of_the_model(mutation):
    caught = [name for name, st, _ in CASES if cases.reorder_plan(st, mutation) != library(st)]
    assert cases.CATCHES[mutation] in caught, (mutation, caught)


def test_a_second_fold_has_nothing_to_do():
    st = cases.state("pieces", 300, 700)
    first = library(st)
    again = dict(st, runs=first["runs"])
    assert library(again) == NOOP == cases.reorder_plan(again)
    # ... and the folded run is a run like any other: a border inside it is refused, a wider range folds it with its neighbours
    assert library(dict(again, **{"from": 300, "count": 300})) == REFUSED
    wider = dict(again, **{"from": 0, "count": 1100})
    assert library(wider) == cases.reorder_plan(wider) == {"runs": [(0, 1100)], "first_block": 0, "end_block": 5}


def test_refused_arguments():
    fn, out = _entry(), ReorderOut()
    assert fn(None, None) == -1
    ok = cases.state("pieces", 0, 557)
    for bad in (dict(ok, runs=[(5, 5)]), dict(ok, runs=[(300, 557), (0, 300)]), dict(ok, runs=[(0, 300), (299, 557)]),
                dict(ok, runs=[(0, 1101)]), dict(ok, slotted=[(9, 3)]), dict(ok, slotted=[(0, 1101)]), dict(ok, uploaded=(1 << 28) + 1)):
        assert fn(C.byref(to_struct(bad)), C.byref(out)) == -1, bad
    s = to_struct(ok)
    s.n_runs = cases.DEBUG_MAX + 1
    assert fn(C.byref(s), C.byref(out)) == -1
