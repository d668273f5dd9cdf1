"""Host model of a draw's host policy (gaussiansplats3d_amd/csrc/draw_plan.cpp), written from the rules in Python floats and
integers - none of the library's fp32 arithmetic.  The policy decides, from the draw before, where the vertex stage runs its block
test, how large the list bins are, whether the previous draw's statistics order the blend's bins (shifted by how many bins),
whether the deep pass runs and where its workgroups sit in the blend's launch.  None of it changes a pixel.

The model REFUSES (AssertionError) inputs on which fp32 and fp64 could decide differently: a motion within 10 % of the limit, a
shift whose fraction lies in [0.4, 0.6], a tiles-per-splat ratio within 1 % of a hysteresis threshold, a visible share within 1 %
of 0.55 or 0.9, a workgroup count within 0.01 of where it truncates.  That is a condition on the cases (draw_plan_cases.py).

Inputs are dicts with the fields of the library's debug entry (draw_plan_cases.FIELDS_IN); matrices are column-major."""
import math
import struct

BIN = 32                              # px: GS_BIN
LIST_SHIFTS = (1, 3, 4, 5)            # 32-, 128-, 256-, 512-px list bins
LIST_TILES_PER_SPLAT = (3.0, 21.0, 80.0)
LIST_SHIFT_SMALL = 1
DEEP_MAX_BINS = 512
DEEP_WGS_PER_SHARE = 0.6
DRAW_FP32 = 0
ORDER_MAX_BINS = 8192


def f32(x):
    """x as the float the library holds (its constants and switches are fp32)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def _bits(values):
    return struct.pack(f"{len(values)}f", *values)


def read_feedback(words):
    """One snapshot of the mapped words.  (A static array cannot tear: a group is invalid only when its serial says 'no draw'.)"""
    w = [int(v) for v in words]
    return {"entries_valid": 1, "serial": w[0], "overflow": int(w[1] != 0), "entries": w[2] | (w[3] << 32),
            "deep_candidates": w[4], "deep_share": w[5],
            "view_valid": int(w[8] != 0), "view_serial": w[8], "visible": w[9], "tiles16": w[10] | (w[11] << 32)}


def adapt_list_shift(current, tiles16, visible):
    """Four levels; up at 1.08 x a threshold of 16-px tiles per visible splat, down below 0.92 x it."""
    if visible == 0:
        return current
    ratio = tiles16 / visible
    for t in LIST_TILES_PER_SPLAT:
        for edge in (1.08 * t, 0.92 * t):
            assert abs(ratio - edge) > 0.01 * edge, f"tiles per splat {ratio} within 1 % of the threshold {edge}"
    level = LIST_SHIFTS.index(current) if current in LIST_SHIFTS[:3] else 3
    while level < 3 and ratio >= 1.08 * LIST_TILES_PER_SPLAT[level]:
        level += 1
    while level > 0 and ratio < 0.92 * LIST_TILES_PER_SPLAT[level - 1]:
        level -= 1
    return LIST_SHIFTS[level]


def entry_room(need):
    room = need + need // 8 + 1024
    assert room < 2 ** 64, "the library's sum is 64-bit"
    return room


def block_test_mode(measured_visible, measured_count, strip, block_cull, no_block_list, block_test_always):
    """1: a kernel of its own; 0: in every workgroup; 2: nowhere."""
    all_live = half_live = False
    if measured_count > 0:
        share = measured_visible / measured_count
        for edge in (0.55, 0.9):
            assert abs(share - edge) > 0.01 * edge, f"visible share {share} within 1 % of {edge}"
        all_live = share > 0.9
        half_live = not all_live and share > 0.55
    test = bool(block_cull) and (not all_live or bool(strip) or bool(block_test_always))
    pretest = test and not no_block_list and (not half_live or bool(strip) or bool(block_test_always))
    return 1 if pretest else (0 if test else 2)


def _window(view, proj, width, height, p):
    """Window position (y up) of the point p, or None when it is not in front of the camera."""
    v = [view[r] * p[0] + view[4 + r] * p[1] + view[8 + r] * p[2] + view[12 + r] for r in range(4)]
    o = [proj[r] * v[0] + proj[4 + r] * v[1] + proj[8 + r] * v[2] + proj[12 + r] * v[3] for r in range(4)]
    if not o[3] > f32(1e-6):
        return None
    return ((o[0] / o[3] * 0.5 + 0.5) * width, (o[1] / o[3] * 0.5 + 0.5) * height)


def _eye(view):
    """The camera's position in the splats' space: -A^-1 b of the modelView [A | b]; None for a singular A."""
    a = [[view[0], view[4], view[8]], [view[1], view[5], view[9]], [view[2], view[6], view[10]]]
    b = [view[12], view[13], view[14]]
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    if not abs(det) > f32(1e-20):
        return None
    eye = []
    for k in range(3):                                     # Cramer's rule for A x = -b
        m = [[(-b[r] if c == k else a[r][c]) for c in range(3)] for r in range(3)]
        dk = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
              m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
        eye.append(dk / det)
    return eye


def plan_schedule(i):
    fb = read_feedback(i["mirror"])
    bins = i["bins_x"] * (i["bin_row_end"] - i["bin_row_begin"])
    fp32 = i["draw_mode"] == DRAW_FP32
    plan = {"blend_bins": bins, "sx": 0, "sy": 0, "deep_factor": i["deep_factor"], "deep_min": i["deep_min"] if fp32 else 0x7FFFFFFF}
    order_ok = (0 < bins <= ORDER_MAX_BINS and i["stats_bins"] == bins and i["stats_row_begin"] == i["bin_row_begin"] and
                i["stats_width_px"] == int(i["width"]) and i["stats_mode"] == i["draw_mode"] and not i["no_blend_order"])
    same_frame = (bool(i["stats_valid"]) and _bits(i["stats_proj"]) == _bits(i["proj"]) and i["stats_width"] == i["width"] and
                  i["stats_height"] == i["height"] and i["stats_count"] == i["count"] and i["stats_list_shift"] == i["list_shift"])
    same_view = same_frame and _bits(i["stats_view"]) == _bits(i["view"])
    if same_frame and not same_view and i["block_cull"] and i["centre_n"] > 0:
        limit = i["order_motion"]
        c = [s / i["centre_n"] for s in i["centre_sum"]]
        was = _window(i["stats_view"], i["stats_proj"], i["stats_width"], i["stats_height"], c)
        now = _window(i["view"], i["proj"], i["width"], i["height"], c)
        if was is not None and now is not None:
            dx, dy = (now[0] - was[0]) / BIN, (now[1] - was[1]) / BIN
            shift_ok = abs(dx) < 4096.0 and abs(dy) < 4096.0 and not i["no_stat_shift"]
            if shift_ok:
                for d in (dx, dy):
                    assert not 0.4 <= d - math.floor(d) <= 0.6, f"a shift of {d} bins: fp32 could round it the other way"
                plan["sx"], plan["sy"] = round(dx), round(dy)
            eye = _eye(i["stats_view"])
            parallax, seen = 0.0, eye is not None
            for t in (0.5, 2.0):
                if not seen:
                    break
                at = _window(i["view"], i["proj"], i["width"], i["height"], [eye[k] + t * (c[k] - eye[k]) for k in range(3)])
                seen = at is not None
                if seen:
                    parallax = max(parallax, math.hypot(at[0] - now[0], at[1] - now[1]))
            moved = (parallax + (0.0 if shift_ok else math.hypot(dx, dy) * BIN)) / max(i["height"], 1.0)
            if seen and not math.isnan(moved):
                if limit > 0.0:
                    assert not 0.9 * limit <= moved <= 1.1 * limit, f"moved {moved} within 10 % of the limit {limit}"
                else:
                    assert moved > 1e-4, f"moved {moved} against a limit of 0: fp32 noise decides"
            same_view = seen and moved <= limit
    plan["order_ok"], plan["same_view"] = int(order_ok), int(same_view)
    deep = order_ok and fp32 and not i["no_deep"] and fb["deep_candidates"] > 0
    plan["deep_pass"] = int(deep)
    plan["order_wg"] = int(order_ok and (same_view or bool(i["blend_order_stale"]) or deep or i["list_shift"] == LIST_SHIFT_SMALL or
                                         (i["draw_serial"] & 7) == 7))
    plan["order_taken"] = int(order_ok and (same_view or bool(i["blend_order_stale"]) or (deep and not i["deep_row_major_on_motion"])))
    return plan


def place_deep_units(plan, bins, cu_count, occupancy, fb, deep_units_last):
    wgs = cu_count * occupancy if plan["deep_pass"] else 0
    at = bins
    if plan["deep_pass"] and plan["order_taken"] and not deep_units_last:
        share = min(fb["deep_share"], 1024) / 1024.0
        by_share = f32(DEEP_WGS_PER_SHARE) * share * wgs + 0.5
        assert abs(by_share - round(by_share)) > 0.01, f"{by_share} workgroups: fp32 could truncate it the other way"
        wgs = min(wgs, max(2 * cu_count, int(by_share)))
        at = min(bins, min(fb["deep_candidates"], DEEP_MAX_BINS) + cu_count + cu_count // 2)
    return {"unit_at": at, "unit_wgs": wgs}


def draw_plan(i):
    """Everything the library's debug entry returns (draw_plan_cases.FIELDS_OUT), by the model."""
    out = dict(read_feedback(i["mirror"]))
    plan = plan_schedule(i)
    out.update(plan)
    out.update(place_deep_units(plan, plan["blend_bins"], i["cu_count"], i["occupancy"], read_feedback(i["mirror"]), i["deep_units_last"]))
    out["room"] = entry_room(i["need"])
    out["list_shift"] = adapt_list_shift(i["list_current"], i["tiles16"], i["visible"])
    out["block_test"] = block_test_mode(i["measured_visible"], i["measured_count"], i["strip"], i["block_cull"], i["no_block_list"],
                                        i["block_test_always"])
    return out
