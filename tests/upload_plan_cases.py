"""The cases of tests/test_upload_plan.py: inputs of the library's pure-host debug entry gs_debug_upload_plan
(csrc/upload_plan.cpp), typed here, and what each case is there to show.

`python tests/upload_plan_cases.py dump FILE` writes the cases' input structs one after the other: what the stand-alone
sanitizer program tests/tools/upload_plan_fuzz.cpp reads."""
import ctypes as C
import itertools
import sys

DEBUG_MAX = 64                                             # UPLOAD_DEBUG_MAX (csrc/upload_plan.hpp)


class PlanIn(C.Structure):                                 # gs_upload_plan_debug_in
    _fields_ = [("n_ranges", C.c_uint32), ("ranges", (C.c_uint32 * 2) * DEBUG_MAX),
                ("from_", C.c_uint32), ("count", C.c_uint32), ("reorder", C.c_uint32),
                ("hold_from", C.c_uint32), ("hold_count", C.c_uint32),
                ("layout_count", C.c_uint32), ("cov_half", C.c_uint32), ("mesh_sh_u8", C.c_uint32), ("sh_degree", C.c_uint32),
                ("source_stages_sh_u8", C.c_uint32)]


class PlanOut(C.Structure):                                # gs_upload_plan_debug_out
    _fields_ = [("n_segments", C.c_uint32), ("segments", (C.c_uint32 * 5) * DEBUG_MAX),
                ("n_before", C.c_uint32), ("before", (C.c_uint32 * 2) * DEBUG_MAX),
                ("n_after", C.c_uint32), ("after", (C.c_uint32 * 2) * DEBUG_MAX),
                ("held", C.c_uint32), ("hold_begin", C.c_uint32), ("hold_end", C.c_uint32),
                ("ncoef", C.c_uint32), ("sh_u8", C.c_uint32),
                ("off_cov", C.c_uint64), ("off_sh", C.c_uint64), ("off_rgba", C.c_uint64), ("bytes", C.c_uint64)]


def make_inputs(ranges=(), start=0, count=0, reorder=1, hold=(0, 0), layout=(1, 0, 0, 0, 0)):
    return {"ranges": [tuple(r) for r in ranges], "from": start, "count": count, "reorder": reorder, "hold_from": hold[0],
            "hold_count": hold[1], "layout_count": layout[0], "cov_half": layout[1], "mesh_sh_u8": layout[2], "sh_degree": layout[3],
            "source_stages_sh_u8": layout[4]}


def to_struct(i):
    s = PlanIn()
    s.n_ranges = len(i["ranges"])
    for k, (b, e) in enumerate(i["ranges"]):
        s.ranges[k][0], s.ranges[k][1] = b, e
    s.from_ = i["from"]
    for name in ("count", "reorder", "hold_from", "hold_count", "layout_count", "cov_half", "mesh_sh_u8", "sh_degree", "source_stages_sh_u8"):
        setattr(s, name, i[name])
    return s


def from_struct(o):
    """A PlanOut as upload_plan_ref.upload_plan spells its answer."""
    rows = lambda a, n: [tuple(int(v) for v in a[k]) for k in range(n)]
    return {"segments": rows(o.segments, o.n_segments), "before": rows(o.before, o.n_before), "after": rows(o.after, o.n_after),
            "held": (int(o.hold_begin), int(o.hold_end)) if o.held else None, "ncoef": int(o.ncoef), "sh_u8": int(o.sh_u8),
            "off_cov": int(o.off_cov), "off_sh": int(o.off_sh), "off_rgba": int(o.off_rgba), "bytes": int(o.bytes)}


THREE = [(100, 200), (300, 400), (500, 600)]
LAYOUT_COUNTS = (1, 21, 256, 257)
LAYOUT_FLAGS = list(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)))      # cov_half, mesh_sh_u8, sh_degree, source_stages_sh_u8


def cases():
    """[(name, inputs, expect)]: expect names what the case is there to show - the model decides everything else as well."""
    c = []
    add = lambda name, expect=None, **kw: c.append((name, make_inputs(**kw), expect or {}))
    # -- cuts
    add("empty_ranges", {"segments": [(10, 50, 1, 0, 1)], "after": [(10, 50)]}, start=10, count=40, hold=(10, 40))
    add("inside_one_range", {"segments": [(120, 180, 0, 0, 1)], "after": THREE, "held": (100, 200)}, ranges=THREE, start=120, count=60, hold=(120, 60))
    add("outside_every_range", {"segments": [(210, 290, 1, 0, 2)], "held": None}, ranges=THREE, start=210, count=80, hold=(210, 80))
    add("ends_on_a_begin", {"segments": [(250, 300, 1, 0, 2)], "after": [(100, 200), (250, 400), (500, 600)]}, ranges=THREE, start=250, count=50)
    add("starts_on_an_end", {"segments": [(200, 250, 1, 0, 1)], "after": [(100, 250), (300, 400), (500, 600)]}, ranges=THREE, start=200, count=50)
    add("fills_a_gap_exactly", {"segments": [(200, 300, 1, 0, 2)], "after": [(100, 400), (500, 600)]}, ranges=THREE, start=200, count=100)
    add("a_whole_range_again", {"segments": [(300, 400, 0, 1, 2)], "after": THREE}, ranges=THREE, start=300, count=100)
    add("crosses_three_ranges", {"segments": [(50, 100, 1, 0, 1), (100, 200, 0, 0, 1), (200, 300, 1, 0, 2), (300, 400, 0, 1, 2),
                                              (400, 500, 1, 1, 2), (500, 550, 0, 1, 3)], "after": [(50, 600)]}, ranges=THREE, start=50, count=500)
    add("starts_inside_a_range_ends_beyond_the_last", {"segments": [(150, 200, 0, 0, 1), (200, 300, 1, 0, 2), (300, 400, 0, 1, 2), (400, 500, 1, 1, 2),
                                                                    (500, 600, 0, 1, 3), (600, 650, 1, 2, 3)], "after": [(100, 650)]},
        ranges=THREE, start=150, count=500)
    add("count_zero", {"segments": [], "after": THREE, "held": (100, 200)}, ranges=THREE, start=150, count=0, hold=(150, 0))
    add("count_zero_no_ranges", {"segments": [], "after": [], "held": None}, start=7, count=0, hold=(7, 0))
    add("ends_at_2_28", {"segments": [((1 << 28) - 1000, 1 << 28, 1, ((1 << 28) - 1000) // 256, 1 << 20)]}, ranges=THREE, start=(1 << 28) - 1000, count=1000)
    add("all_2_28", {"after": [(0, 1 << 28)]}, ranges=THREE, start=0, count=1 << 28, hold=(0, 1 << 28))
    add("inputs_overlap_and_touch", {"before": [(0, 300), (400, 500)]}, ranges=[(200, 300), (0, 100), (100, 250), (400, 450), (450, 500)], start=300, count=100)
    # 0xFFFFFFF0 + 0x20 is 0x10 in 32 bits: "at or before the range's end" only if the sum is allowed to wrap
    add("holding_sum_past_2_32", {"held": None}, ranges=[(0, 1 << 28)], hold=(0xFFFFFFF0, 0x20))
    add("holding_sum_past_2_32_low_range", {"held": None}, ranges=[(0, 0x100)], hold=(0xFFFFFFF0, 0x20))
    add("holding_up_to_the_end", {"held": (300, 400)}, ranges=THREE, hold=(350, 50))
    add("holding_one_past_the_end", {"held": None}, ranges=THREE, hold=(350, 51))
    add("holding_across_a_gap", {"held": None}, ranges=THREE, hold=(150, 200))
    # -- box spans
    add("inside_one_block", {"segments": [(300, 500, 1, 1, 2)]}, start=300, count=200)
    add("ends_on_a_block_border", {"segments": [(300, 512, 1, 1, 2)]}, start=300, count=212)
    add("starts_on_a_block_border", {"segments": [(512, 513, 1, 2, 3)]}, start=512, count=1)
    #  the splats keep slots anywhere in the range that held them: every block of [100, 1900) is redone, not 2 .. 3
    add("not_fresh_inside_a_wide_range", {"segments": [(600, 700, 0, 0, 8)]}, ranges=[(100, 1900)], start=600, count=100)
    add("not_fresh_then_fresh", {"segments": [(1800, 1900, 0, 0, 8), (1900, 2100, 1, 7, 9)]}, ranges=[(100, 1900)], start=1800, count=300)
    add("keep_order_is_always_fresh", {"segments": [(600, 700, 1, 2, 3)]}, ranges=[(100, 1900)], start=600, count=100, reorder=0)
    add("keep_order_still_cuts", {"segments": [(50, 100, 1, 0, 1), (100, 150, 1, 0, 1)]}, ranges=[(100, 1900)], start=50, count=100, reorder=0)
    # -- layout
    for n in LAYOUT_COUNTS:
        for f in LAYOUT_FLAGS:
            add("layout_%d_half%d_u8%d_sh%d_src%d" % ((n,) + f), layout=(n,) + f)
    return c


def dump(path):
    with open(path, "wb") as f:
        for _, inputs, _ in cases():
            f.write(bytes(to_struct(inputs)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit("usage: upload_plan_cases.py dump FILE")
