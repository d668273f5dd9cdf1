"""Host model of plan_reorder (csrc/upload_plan.cpp) and the named cases tests/test_reorder_plan.py holds the library to: what
gs_mesh_reorder decides before it touches the device, as bitmaps over the positions - one flag "owns a slot" and one run number
per position.  Nothing here shares a line of reasoning with the library's interval arithmetic.

`mutation` names one deliberate mistake (MUTATIONS); every one of them is told from the model by a case named in CATCHES."""
import ctypes as C

import numpy as np

BLOCK = 256                                                # UPLOAD_BLOCK
DEBUG_MAX = 64                                             # UPLOAD_DEBUG_MAX
REFUSED, NOOP = "refused", "noop"
MUTATIONS = ("begin_border_off_by_one", "end_border_ignored", "hole_ignored", "touching_runs_merge_outside", "end_block_rounded_down",
             "first_block_rounded_up", "a_single_run_is_folded", "uploaded_not_checked")

Rows2 = (C.c_uint32 * 2) * DEBUG_MAX


class ReorderIn(C.Structure):                              # gs_reorder_plan_debug_in
    _fields_ = [("n_runs", C.c_uint32), ("runs", Rows2), ("n_slotted", C.c_uint32), ("slotted", Rows2),
                ("uploaded", C.c_uint32), ("reorder", C.c_uint32), ("from_", C.c_uint32), ("count", C.c_uint32)]


class ReorderOut(C.Structure):                             # gs_reorder_plan_debug_out
    _fields_ = [("refused", C.c_uint32), ("noop", C.c_uint32), ("n_runs", C.c_uint32), ("runs", Rows2),
                ("first_block", C.c_uint32), ("end_block", C.c_uint32)]


def _segments(values):
    """[(begin, end, value)] of the maximal constant stretches of a vector"""
    if values.size == 0:
        return []
    edges = np.flatnonzero(np.diff(values)) + 1
    begins = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [values.size]])
    return [(int(b), int(e), int(values[b])) for b, e in zip(begins, ends)]


def reorder_plan(state, mutation=None):
    """state: {"runs": [(b, e)], "slotted": [(b, e)], "uploaded", "reorder", "from", "count"} -> REFUSED, NOOP or
    {"runs": [(b, e)], "first_block", "end_block"}."""
    up, start, count = state["uploaded"], state["from"], state["count"]
    if count == 0:
        return NOOP
    end = start + count
    if end > up and mutation != "uploaded_not_checked":
        return REFUSED
    if not state["reorder"]:
        return NOOP
    size = max(up, end) + 2
    slot = np.zeros(size, bool)
    for b, e in state["slotted"]:
        slot[b:e] = True
    run_of = np.zeros(size, np.int64)
    for k, (b, e) in enumerate(state["runs"]):
        run_of[b:e] = k + 1
    if not slot[start:end].all() and mutation != "hole_ignored":
        return REFUSED
    borders = [start + 1 if mutation == "begin_border_off_by_one" else start] + ([] if mutation == "end_border_ignored" else [end])
    if any(at > 0 and run_of[at - 1] and run_of[at - 1] == run_of[at] for at in borders):   # the same run on both sides
        return REFUSED
    inside = set(int(v) for v in run_of[start:end] if v)
    if len(inside) <= 1 and mutation != "a_single_run_is_folded":
        return NOOP
    run_of[start:end] = len(state["runs"]) + 1             # one run
    if mutation == "touching_runs_merge_outside":
        run_of = (run_of > 0).astype(np.int64)
    runs = [(b, e) for b, e, v in _segments(run_of) if v]
    first = -(-start // BLOCK) if mutation == "first_block_rounded_up" else start // BLOCK
    last = end // BLOCK if mutation == "end_block_rounded_down" else -(-end // BLOCK)
    return {"runs": runs, "first_block": first, "end_block": last}


def state(kind, start, count):
    s = {"pieces": {"runs": [(0, 300), (300, 557), (557, 1000), (1000, 1100)], "slotted": [(0, 1100)], "uploaded": 1100, "reorder": 1},
         "blocks": {"runs": [(0, 256), (256, 512), (512, 768), (768, 900)], "slotted": [(0, 900)], "uploaded": 900, "reorder": 1},
         "forty": {"runs": [(25 * k, 25 * k + 25) for k in range(40)], "slotted": [(0, 1000)], "uploaded": 1000, "reorder": 1},
         "holes": {"runs": [(100, 200), (300, 400), (400, 500)], "slotted": [(100, 200), (300, 500)], "uploaded": 500, "reorder": 1},
         "keep_order": {"runs": [], "slotted": [(0, 1000)], "uploaded": 1000, "reorder": 0}}[kind]
    return dict(s, **{"from": start, "count": count})


# (name, state, what the case is there to show: REFUSED, NOOP or some fields of the plan)
CASES = [
    # -- how many runs the range holds
    ("one_run", state("pieces", 300, 257), NOOP),
    ("the_last_run_alone", state("pieces", 1000, 100), NOOP),
    ("two_runs", state("pieces", 0, 557), {"runs": [(0, 557), (557, 1000), (1000, 1100)], "first_block": 0, "end_block": 3}),
    ("every_run", state("pieces", 0, 1100), {"runs": [(0, 1100)], "first_block": 0, "end_block": 5}),
    ("forty_runs", state("forty", 0, 1000), {"runs": [(0, 1000)], "first_block": 0, "end_block": 4}),
    ("thirty_eight_of_forty", state("forty", 25, 950), {"runs": [(0, 25), (25, 975), (975, 1000)], "first_block": 0, "end_block": 4}),
    ("the_middle_two_of_four", state("pieces", 300, 700), {"runs": [(0, 300), (300, 1000), (1000, 1100)], "first_block": 1, "end_block": 4}),
    # -- borders on and inside a run
    ("begin_inside_a_run", state("pieces", 10, 547), REFUSED),
    ("begin_one_before_a_border", state("pieces", 299, 701), REFUSED),
    ("begin_one_behind_a_border", state("pieces", 301, 699), REFUSED),
    ("end_inside_a_run", state("pieces", 0, 400), REFUSED),
    ("end_one_before_a_border", state("pieces", 0, 556), REFUSED),
    ("end_one_behind_a_border", state("pieces", 0, 558), REFUSED),
    ("end_inside_the_last_run", state("pieces", 557, 542), REFUSED),
    # -- re-uploaded (non-fresh) splats keep their slots inside the run: their range is no run of its own
    ("a_reuploaded_range_inside_a_run", state("pieces", 310, 100), REFUSED),
    # -- never-uploaded positions
    ("a_hole_in_the_middle", state("holes", 100, 400), REFUSED),
    ("a_hole_at_the_begin", state("holes", 0, 200), REFUSED),
    ("one_position_of_a_hole", state("holes", 299, 201), REFUSED),
    ("beside_the_hole", state("holes", 300, 200), {"runs": [(100, 200), (300, 500)], "first_block": 1, "end_block": 2}),
    ("the_hole_alone", state("holes", 200, 100), REFUSED),
    # -- the uploaded count
    ("ends_beyond_uploaded", state("pieces", 557, 600), REFUSED),
    ("one_beyond_uploaded", state("pieces", 0, 1101), REFUSED),
    ("wholly_beyond_uploaded", state("pieces", 1100, 10), REFUSED),
    ("sum_past_2_32", state("pieces", 0xFFFFFFF0, 0x20), REFUSED),
    ("count_zero", state("pieces", 10, 0), NOOP),
    ("count_zero_beyond_uploaded", state("pieces", 5000, 0), NOOP),
    # -- a mesh that keeps upload order
    ("reorder_off", state("keep_order", 0, 1000), NOOP),
    ("reorder_off_a_piece", state("keep_order", 10, 5), NOOP),
    ("reorder_off_given_runs", dict(state("keep_order", 0, 1000), runs=[(0, 400), (400, 1000)]), NOOP),
    ("reorder_off_beyond_uploaded", state("keep_order", 900, 101), REFUSED),
    # -- the storage blocks that get new boxes
    ("borders_inside_storage_blocks", state("pieces", 300, 700), {"first_block": 1, "end_block": 4}),
    ("borders_on_block_edges", state("blocks", 256, 512), {"runs": [(0, 256), (256, 768), (768, 900)], "first_block": 1, "end_block": 3}),
    ("end_in_the_last_partial_block", state("blocks", 512, 388), {"runs": [(0, 256), (256, 512), (512, 900)], "first_block": 2, "end_block": 4}),
]

# the case that tells each mutation from the model
CATCHES = {"begin_border_off_by_one": "begin_one_before_a_border", "end_border_ignored": "end_inside_a_run", "hole_ignored": "a_hole_in_the_middle",
           "touching_runs_merge_outside": "the_middle_two_of_four", "end_block_rounded_down": "borders_inside_storage_blocks",
           "first_block_rounded_up": "borders_inside_storage_blocks", "a_single_run_is_folded": "one_run",
           "uploaded_not_checked": "reorder_off_beyond_uploaded"}
