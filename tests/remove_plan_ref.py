"""Host model of plan_remove (csrc/upload_plan.cpp): what gs_mesh_remove / gs_sorter_remove do to the numbering, as bitmaps over
the positions [0, max_count) - one flag "owns a slot", one run number, one flag "goes away" per position.  Nothing here shares a
line of reasoning with the library's interval arithmetic.

`mutation` names one deliberate mistake (MUTATIONS): tests/test_remove_plan.py shows that its cases tell each of them from the
model."""
import numpy as np

MAX_RANGES = 32                                            # REMOVE_MAX_RANGES
BLOCK = 256                                                # UPLOAD_BLOCK
MUTATIONS = ("no_run_rule", "run_rule_ignores_the_end", "touching_runs_merge", "no_clip_to_uploaded", "shift_excludes_own_cut",
             "first_block_of_the_last_cut", "touching_ranges_refused", "slotted_not_merged")


def _segments(values):
    """[(begin, end, value)] of the maximal constant stretches of a vector"""
    if values.size == 0:
        return []
    edges = np.flatnonzero(np.diff(values)) + 1
    begins = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [values.size]])
    return [(int(b), int(e), int(values[b])) for b, e in zip(begins, ends)]


def remove_plan(state, mutation=None):
    """state: {"runs": [(b, e)], "slotted": [(b, e)], "uploaded", "max_count", "reorder", "ranges": [(from, count)]} ->
    None (refused) or {"moves": [(begin, end, shift)], "runs", "slotted", "removed", "uploaded", "first_block"}."""
    ranges, up, cap = state["ranges"], state["uploaded"], state["max_count"]
    if not 1 <= len(ranges) <= MAX_RANGES:
        return None
    gone = np.zeros(cap, bool)
    prev_end = 0
    for start, count in ranges:
        if count == 0 or start + count > cap:
            return None
        if start < prev_end or (mutation == "touching_ranges_refused" and start == prev_end and prev_end):
            return None
        prev_end = start + count
        gone[start:start + count] = True
    run_of = np.zeros(cap, np.int64)
    for k, (b, e) in enumerate(state["runs"] if state["reorder"] else []):
        run_of[b:e] = k + 1
    slot = np.zeros(cap, bool)
    for b, e in state["slotted"]:
        slot[b:e] = True
    if state["reorder"] and mutation != "no_run_rule":     # no border of a range has the same run on both sides
        borders = [s for s, _ in ranges] + ([] if mutation == "run_rule_ignores_the_end" else [s + c for s, c in ranges])
        if any(0 < at < cap and run_of[at - 1] and run_of[at - 1] == run_of[at] for at in borders):
            return None
    if mutation != "no_clip_to_uploaded":
        gone[up:] = False
    live = np.flatnonzero(~gone[:up])                      # the survivors, in order
    removed = int(gone.sum())                              # (positions beyond the uploaded count were never there)
    shift = live - np.arange(live.size)                    # survivor i lands on i - (removed positions below i)
    if mutation == "shift_excludes_own_cut":
        shift = np.maximum(shift - 1, 0)
    moves = [(int(live[b]), int(live[e - 1]) + 1, s) for b, e, s in _segments(shift) if s > 0]
    runs = []
    kept_run = run_of[live]
    for b, e, r in _segments(kept_run):
        if r:
            runs.append((b, e))
    if mutation == "touching_runs_merge":
        runs = [(b, e) for b, e, v in _segments((kept_run > 0).astype(np.int64)) if v]
    kept_slot = slot[live].astype(np.int64)
    slotted = [(b, e) for b, e, v in _segments(kept_slot) if v]
    if mutation == "slotted_not_merged":                   # one range per range before, even where two now touch
        slotted = []
        for b, e in state["slotted"]:
            at = np.flatnonzero((live >= b) & (live < e))  # (consecutive: the survivors keep their order)
            if at.size:
                slotted.append((int(at[0]), int(at[-1]) + 1))
    cut_begins = [s for s, _ in ranges if s < up]
    first = 0
    if cut_begins:
        first = (cut_begins[-1] if mutation == "first_block_of_the_last_cut" else cut_begins[0]) // BLOCK
    return {"moves": moves, "runs": runs, "slotted": slotted, "removed": removed, "uploaded": up - removed, "first_block": first}


def after(state, plan):
    """the state a following call sees"""
    return {"runs": plan["runs"], "slotted": plan["slotted"], "uploaded": plan["uploaded"], "max_count": state["max_count"],
            "reorder": state["reorder"]}
