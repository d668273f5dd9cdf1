"""The host plan of gs_mesh_remove / gs_sorter_remove (csrc/upload_plan.cpp, plan_remove) held to its bitmap model
(remove_plan_ref.py) through the library's pure-host debug entry gs_debug_remove_plan: no GPU.  The plan decides which calls are
refused, which spans of survivors move down by how much, which Morton runs and slotted ranges are left (shifted), the uploaded
count afterwards and the first storage block whose boxes are redone."""
import ctypes as C

import pytest

import gaussiansplats3d_amd as g
import remove_plan_ref as ref

DEBUG_MAX = 64                                             # UPLOAD_DEBUG_MAX (csrc/upload_plan.hpp)
Rows2 = (C.c_uint32 * 2) * DEBUG_MAX


class RemoveIn(C.Structure):                               # gs_remove_plan_debug_in
    _fields_ = [("n_runs", C.c_uint32), ("runs", Rows2), ("n_slotted", C.c_uint32), ("slotted", Rows2),
                ("uploaded", C.c_uint32), ("max_count", C.c_uint32), ("reorder", C.c_uint32),
                ("n_ranges", C.c_uint32), ("ranges", Rows2)]


class RemoveOut(C.Structure):                              # gs_remove_plan_debug_out
    _fields_ = [("refused", C.c_uint32), ("n_moves", C.c_uint32), ("moves", (C.c_uint32 * 3) * DEBUG_MAX),
                ("n_runs", C.c_uint32), ("runs", Rows2), ("n_slotted", C.c_uint32), ("slotted", Rows2),
                ("removed", C.c_uint32), ("uploaded", C.c_uint32), ("first_block", C.c_uint32)]


def _entry():
    fn = g.load().gs_debug_remove_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(RemoveIn), C.POINTER(RemoveOut)]
    return fn


def to_struct(state):
    s = RemoveIn()
    for name in ("runs", "slotted", "ranges"):
        setattr(s, "n_" + name, len(state[name]))
        for k, (a, b) in enumerate(state[name][:DEBUG_MAX]):
            getattr(s, name)[k][0], getattr(s, name)[k][1] = a, b
    s.uploaded, s.max_count, s.reorder = state["uploaded"], state["max_count"], state["reorder"]
    return s


def library(state):
    out = RemoveOut()
    assert _entry()(C.byref(to_struct(state)), C.byref(out)) == 0
    if out.refused:
        return None
    rows = lambda a, n: [tuple(int(v) for v in a[k]) for k in range(n)]
    return {"moves": rows(out.moves, out.n_moves), "runs": rows(out.runs, out.n_runs), "slotted": rows(out.slotted, out.n_slotted),
            "removed": int(out.removed), "uploaded": int(out.uploaded), "first_block": int(out.first_block)}


def state(kind, ranges):
    s = {"morton": {"runs": [(0, 300), (300, 557), (557, 1000)], "slotted": [(0, 1000)], "uploaded": 1000, "max_count": 1200, "reorder": 1},
         "holes": {"runs": [(100, 200), (300, 400), (400, 500)], "slotted": [(100, 200), (300, 500)], "uploaded": 500, "max_count": 600, "reorder": 1},
         "keep_order": {"runs": [], "slotted": [(0, 400), (600, 1000)], "uploaded": 1000, "max_count": 1000, "reorder": 0},
         "sorter": {"runs": [], "slotted": [], "uploaded": 1000, "max_count": 1000, "reorder": 0}}[kind]
    return dict(s, ranges=list(ranges))


REFUSED = "refused"
CASES = [
    # -- whole runs
    ("first", state("morton", [(0, 300)]), {"moves": [(300, 1000, 300)], "runs": [(0, 257), (257, 700)], "slotted": [(0, 700)], "uploaded": 700, "first_block": 0}),
    ("middle", state("morton", [(300, 257)]), {"moves": [(557, 1000, 257)], "runs": [(0, 300), (300, 743)], "first_block": 1}),
    ("last", state("morton", [(557, 443)]), {"moves": [], "runs": [(0, 300), (300, 557)], "uploaded": 557, "first_block": 2}),
    ("first_and_last", state("morton", [(0, 300), (557, 443)]), {"moves": [(300, 557, 300)], "runs": [(0, 257)], "uploaded": 257, "first_block": 0}),
    ("two_ranges_that_touch", state("morton", [(0, 300), (300, 257)]), {"moves": [(557, 1000, 557)], "runs": [(0, 443)]}),
    ("one_range_over_two_runs", state("morton", [(0, 557)]), {"moves": [(557, 1000, 557)], "runs": [(0, 443)]}),
    ("everything", state("morton", [(0, 1000)]), {"moves": [], "runs": [], "slotted": [], "uploaded": 0, "removed": 1000}),
    # -- the uploaded count
    ("ends_beyond_uploaded", state("morton", [(557, 643)]), {"removed": 443, "uploaded": 557}),
    ("wholly_beyond_uploaded", state("morton", [(1000, 200)]), {"removed": 0, "uploaded": 1000, "moves": [], "runs": [(0, 300), (300, 557), (557, 1000)]}),
    ("behind_and_beyond", state("morton", [(0, 300), (1100, 100)]), {"removed": 300, "moves": [(300, 1000, 300)]}),
    # -- the run rule
    ("begin_splits_a_run", state("morton", [(250, 307)]), REFUSED),
    ("end_splits_a_run", state("morton", [(300, 100)]), REFUSED),
    ("inside_one_run", state("morton", [(10, 5)]), REFUSED),
    ("two_ranges_meet_inside_a_run", state("morton", [(0, 100), (100, 200)]), REFUSED),
    ("end_splits_the_last_run", state("morton", [(0, 999)]), REFUSED),
    # -- holes: never-uploaded positions go as they like, the ranges that touch afterwards are one, the runs are not
    ("a_piece_of_the_first_hole", state("holes", [(0, 50)]), {"moves": [(50, 500, 50)], "runs": [(50, 150), (250, 350), (350, 450)], "slotted": [(50, 150), (250, 450)]}),
    ("a_piece_of_the_middle_hole", state("holes", [(220, 30)]), {"moves": [(250, 500, 30)], "runs": [(100, 200), (270, 370), (370, 470)]}),
    ("the_whole_middle_hole", state("holes", [(200, 100)]), {"runs": [(100, 200), (200, 300), (300, 400)], "slotted": [(100, 400)]}),
    ("a_run_between_hole_and_run", state("holes", [(300, 100)]), {"runs": [(100, 200), (300, 400)], "slotted": [(100, 200), (300, 400)], "first_block": 1}),
    ("hole_and_run_in_one_range", state("holes", [(200, 200)]), {"runs": [(100, 200), (200, 300)], "slotted": [(100, 300)]}),
    ("a_run_of_the_holes_split", state("holes", [(150, 100)]), REFUSED),
    # -- no runs: any range
    ("keep_order_anywhere", state("keep_order", [(10, 5), (700, 100)]), {"moves": [(15, 700, 5), (800, 1000, 105)], "runs": [], "slotted": [(0, 395), (595, 895)]}),
    ("keep_order_closes_the_gap", state("keep_order", [(400, 200)]), {"slotted": [(0, 800)]}),
    ("keep_order_given_runs_has_none", dict(state("keep_order", [(10, 5)]), runs=[(0, 400)]), {"runs": []}),
    ("sorter_three_ranges", state("sorter", [(0, 1), (1, 1), (998, 2)]), {"moves": [(2, 998, 2)], "uploaded": 996, "slotted": []}),
    ("thirty_two_ranges", state("sorter", [(4 * k, 2) for k in range(32)]), {"removed": 64}),
    # -- malformed calls
    ("no_ranges", state("morton", []), REFUSED),
    ("thirty_three_ranges", state("sorter", [(4 * k, 2) for k in range(33)]), REFUSED),
    ("an_empty_range", state("morton", [(0, 300), (557, 0)]), REFUSED),
    ("descending", state("morton", [(557, 443), (0, 300)]), REFUSED),
    ("overlapping", state("sorter", [(0, 300), (299, 10)]), REFUSED),
    ("beyond_the_capacity", state("morton", [(557, 644)]), REFUSED),
    ("sum_past_2_32", state("sorter", [(0xFFFFFFF0, 0x20)]), REFUSED),
]


def test_the_case_names_are_unique():
    assert len(CASES) == len(set(name for name, _, _ in CASES))


@pytest.mark.parametrize("name,st,expect", CASES, ids=[c[0] for c in CASES])
def test_library_decides_as_the_model(name, st, expect):
    want, got = ref.remove_plan(st), library(st)
    assert got == want, (got, want)
    if expect == REFUSED:
        assert got is None
        return
    for key, value in expect.items():                      # what the case is there to show
        assert got[key] == value, (key, got[key], value)
    # the moves and the untouched head are the survivors, packed: each move lands right behind what is below it
    end = st["ranges"][0][0] if got["removed"] else got["uploaded"]
    for b, e, shift in got["moves"]:
        assert b < e and shift > 0 and b - shift == end
        end = e - shift
    assert end == got["uploaded"] == st["uploaded"] - got["removed"] or not got["moves"]
    assert all(b < e for b, e in got["runs"]) and all(a[1] <= b[0] for a, b in zip(got["runs"], got["runs"][1:]))
    assert all(b < e for b, e in got["slotted"]) and all(a[1] < b[0] for a, b in zip(got["slotted"], got["slotted"][1:]))
    assert all(e <= got["uploaded"] for _, e in got["runs"] + got["slotted"])


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_the_cases_catch_every_mutation_of_the_model(mutation):
    caught = [name for name, st, _ in CASES if ref.remove_plan(st, mutation) != library(st)]
    assert caught, mutation


def test_two_removals_in_a_row():
    """The second call is planned on the runs and ranges the first one left."""
    st = state("morton", [(300, 257)])
    first = library(st)
    assert first == ref.remove_plan(st) and first["runs"] == [(0, 300), (300, 743)]
    st2 = dict(ref.after(st, first), ranges=[(0, 300)])
    second = library(st2)
    assert second == ref.remove_plan(st2)
    assert second == {"moves": [(300, 743, 300)], "runs": [(0, 443)], "slotted": [(0, 443)], "removed": 300, "uploaded": 443, "first_block": 0}
    # the old border of the removed run is no border any more: 300 now lies inside the one run left
    assert library(dict(ref.after(st2, second), ranges=[(300, 143)])) is None
    # ... and with holes: the ranges merge, the runs keep their borders, and each can still go on its own
    st = state("holes", [(200, 100)])
    first = library(st)
    st2 = dict(ref.after(st, first), ranges=[(200, 100)])
    second = library(st2)
    assert second == ref.remove_plan(st2) and second["runs"] == [(100, 200), (200, 300)] and second["slotted"] == [(100, 300)]


def test_refused_arguments():
    fn, out = _entry(), RemoveOut()
    assert fn(None, None) == -1
    ok = state("morton", [(0, 300)])
    for bad in (dict(ok, runs=[(5, 5)]), dict(ok, runs=[(300, 557), (0, 300)]), dict(ok, runs=[(0, 300), (299, 557)]),
                dict(ok, runs=[(0, 1001)]), dict(ok, slotted=[(9, 3)]), dict(ok, slotted=[(0, 1001)]), dict(ok, uploaded=1201),
                dict(ok, max_count=(1 << 28) + 1)):
        assert fn(C.byref(to_struct(bad)), C.byref(out)) == -1, bad
    s = to_struct(ok)
    s.n_ranges = DEBUG_MAX + 1
    assert fn(C.byref(s), C.byref(out)) == -1
