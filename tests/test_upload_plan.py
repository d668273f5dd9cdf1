"""The host policy of an upload (csrc/upload_plan.cpp) held to its host model (upload_plan_ref.py, a bitmap of the slotted splats)
through the library's pure-host debug entry: no GPU.  The policy decides which splats of an upload receive storage slots and
which keep theirs, which storage blocks get new boxes, which ranges gs_mesh_bounds and the 8-bit-SH / scene-index uploads accept,
and where a segment's arrays sit in the staging buffer the decode kernels write."""
import ctypes as C

import pytest

import gaussiansplats3d_amd as g
import upload_plan_cases as uc
import upload_plan_ref as ref

CASES = uc.cases()


def _entry():
    fn = g.load().gs_debug_upload_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(uc.PlanIn), C.POINTER(uc.PlanOut)]
    return fn


def library(inputs):
    s, out = uc.to_struct(inputs), uc.PlanOut()
    assert _entry()(C.byref(s), C.byref(out)) == 0
    return uc.from_struct(out)


def well_formed(ranges):
    """non-empty, sorted by begin, disjoint and never adjacent"""
    return all(b < e for b, e in ranges) and all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))


def test_the_case_names_are_unique():
    assert len(CASES) == len(set(name for name, _, _ in CASES))


@pytest.mark.parametrize("name,inputs,expect", CASES, ids=[c[0] for c in CASES])
def test_library_decides_as_the_model(name, inputs, expect):
    want = ref.upload_plan(inputs)
    got = library(inputs)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    for key, value in expect.items():                      # what the case is there to show
        assert got[key] == value, (key, got[key], value)
    assert well_formed(got["before"]) and well_formed(got["after"])
    start, end = inputs["from"], inputs["from"] + inputs["count"]
    segs = got["segments"]
    if start < end:                                        # the segments tile [from, end): no gap, no overlap, none empty
        assert segs[0][0] == start and segs[-1][1] == end and all(b < e for b, e, *_ in segs)
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert any(b <= start and end <= e for b, e in got["after"])      # ... and afterwards one range holds all of it
    else:
        assert segs == [] and got["after"] == got["before"]
    for b, e, fresh, b0, b1 in segs:                       # a segment's own blocks are always among those redone
        assert b0 <= b // 256 and -(-e // 256) <= b1


@pytest.mark.parametrize("count", uc.LAYOUT_COUNTS)
@pytest.mark.parametrize("flags", uc.LAYOUT_FLAGS, ids=["half%d_u8%d_sh%d_src%d" % f for f in uc.LAYOUT_FLAGS])
def test_layout_planes_fit_and_are_aligned(count, flags):
    cov_half, mesh_sh_u8, sh_degree, src = flags
    got = library(uc.make_inputs(layout=(count,) + flags))
    assert {k: got[k] for k in ("ncoef", "sh_u8", "off_cov", "off_sh", "off_rgba", "bytes")} == ref.upload_layout(count, *flags)
    assert got["ncoef"] == (0 if sh_degree == 0 or (mesh_sh_u8 and not src) else (9, 24)[sh_degree - 1])
    assert got["sh_u8"] == int(bool(mesh_sh_u8 and got["ncoef"]))
    planes = [(0, count * 12), (got["off_cov"], count * (12 if cov_half else 24)),
              (got["off_sh"], count * got["ncoef"] * (1 if got["sh_u8"] else 2)), (got["off_rgba"], count * 4)]
    for (off, size), (nxt, _) in zip(planes, planes[1:] + [(got["bytes"], 0)]):
        assert off % 256 == 0 and off + size <= nxt and off + size <= got["bytes"], (off, size, nxt)


def test_refused_arguments():
    fn = _entry()
    assert fn(None, None) == -1
    out = uc.PlanOut()
    for bad in (uc.make_inputs(ranges=[(5, 5)]), uc.make_inputs(ranges=[(9, 3)]), uc.make_inputs(start=1 << 28, count=1),
                uc.make_inputs(start=0xFFFFFFFF, count=0xFFFFFFFF), uc.make_inputs(ranges=[(0, (1 << 28) + 1)])):
        assert fn(C.byref(uc.to_struct(bad)), C.byref(out)) == -1, bad
    s = uc.to_struct(uc.make_inputs())
    s.n_ranges = uc.DEBUG_MAX + 1
    assert fn(C.byref(s), C.byref(out)) == -1
    comb = [(4 * k, 4 * k + 2) for k in range(40)]         # 81 segments do not fit the entry's 64 rows
    assert fn(C.byref(uc.to_struct(uc.make_inputs(ranges=comb, start=1, count=160))), C.byref(out)) == -1


def test_a_sequence_of_uploads_keeps_the_model():
    """The five uploads of tests/test_gpu_upload_plan.py, each planned on the ranges the one before left."""
    ranges, shown = [], []
    for start, end in [(100, 300), (500, 700), (0, 600), (700, 1000), (650, 750)]:
        got = library(uc.make_inputs(ranges=ranges, start=start, count=end - start))
        assert got["segments"] == ref.plan_upload(ranges, start, end - start, 1) and got["before"] == ranges
        ranges = got["after"]
        shown.append(([s[:3] for s in got["segments"]], ranges))
    assert shown[2] == ([(0, 100, 1), (100, 300, 0), (300, 500, 1), (500, 600, 0)], [(0, 700)])
    assert shown[3] == ([(700, 1000, 1)], [(0, 1000)])
    assert shown[4] == ([(650, 750, 0)], [(0, 1000)]) and got["segments"][0][3:] == (0, 4)
