"""The cases of tests/test_draw_plan.py: inputs of the library's pure-host debug entry gs_debug_draw_plan (csrc/draw_plan.cpp),
typed here, and what each case is there to show.  Every case has to pass the host model's own check that fp32 and fp64 cannot
decide it differently (draw_plan_ref.py); none may be left out.

`python tests/draw_plan_cases.py dump FILE` writes the cases' input structs one after the other: what the stand-alone sanitizer
program tests/tools/draw_plan_fuzz.cpp reads."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import draw_plan_ref as ref  # noqa: E402
from gaussiansplats3d_amd import camera  # noqa: E402

MIRROR_WORDS = 16


class PlanIn(C.Structure):                                 # gs_draw_plan_debug_in (csrc/draw_plan.hpp)
    _fields_ = [("centre_sum", C.c_double * 3), ("centre_n", C.c_uint64), ("tiles16", C.c_uint64), ("need", C.c_uint64),
                ("mirror", C.c_uint32 * MIRROR_WORDS),
                ("stats_valid", C.c_uint32), ("stats_bins", C.c_uint32), ("stats_row_begin", C.c_uint32), ("stats_width_px", C.c_uint32),
                ("stats_mode", C.c_uint32),
                ("stats_view", C.c_float * 16), ("stats_proj", C.c_float * 16), ("stats_width", C.c_float), ("stats_height", C.c_float),
                ("stats_count", C.c_uint32), ("stats_list_shift", C.c_uint32),
                ("view", C.c_float * 16), ("proj", C.c_float * 16), ("width", C.c_float), ("height", C.c_float),
                ("count", C.c_uint32), ("list_shift", C.c_uint32), ("bins_x", C.c_uint32), ("bin_row_begin", C.c_uint32),
                ("bin_row_end", C.c_uint32), ("block_cull", C.c_uint32), ("draw_mode", C.c_uint32), ("draw_serial", C.c_uint32),
                ("no_deep", C.c_uint32),
                ("deep_min", C.c_uint32), ("deep_factor", C.c_uint32), ("no_blend_order", C.c_uint32), ("order_motion", C.c_float),
                ("no_stat_shift", C.c_uint32), ("blend_order_stale", C.c_uint32), ("deep_row_major_on_motion", C.c_uint32),
                ("deep_units_last", C.c_uint32),
                ("cu_count", C.c_uint32), ("occupancy", C.c_uint32), ("list_current", C.c_uint32), ("visible", C.c_uint32),
                ("measured_visible", C.c_uint32), ("measured_count", C.c_uint32), ("strip", C.c_uint32), ("no_block_list", C.c_uint32),
                ("block_test_always", C.c_uint32)]


class PlanOut(C.Structure):                                # gs_draw_plan_debug_out
    _fields_ = [("entries", C.c_uint64), ("tiles16", C.c_uint64), ("room", C.c_uint64),
                ("entries_valid", C.c_uint32), ("serial", C.c_uint32), ("overflow", C.c_uint32), ("deep_candidates", C.c_uint32),
                ("deep_share", C.c_uint32), ("view_valid", C.c_uint32), ("view_serial", C.c_uint32), ("visible", C.c_uint32),
                ("blend_bins", C.c_uint32), ("order_ok", C.c_uint32), ("same_view", C.c_uint32), ("sx", C.c_int32), ("sy", C.c_int32),
                ("order_wg", C.c_uint32), ("order_taken", C.c_uint32), ("deep_pass", C.c_uint32), ("deep_min", C.c_uint32),
                ("deep_factor", C.c_uint32), ("unit_at", C.c_uint32), ("unit_wgs", C.c_uint32), ("list_shift", C.c_uint32),
                ("block_test", C.c_int32)]


FIELDS_IN = [f[0] for f in PlanIn._fields_]
FIELDS_OUT = [f[0] for f in PlanOut._fields_]


def to_struct(i):
    s = PlanIn()
    for name in FIELDS_IN:
        v = i[name]
        if isinstance(v, (list, tuple, np.ndarray)):
            for k, x in enumerate(v):
                getattr(s, name)[k] = x
        else:
            setattr(s, name, v)
    return s


def from_struct(s):
    """The inputs as the library reads them (fp32 fields rounded to fp32): what the model is given."""
    return {name: (list(getattr(s, name)) if hasattr(getattr(s, name), "__len__") else getattr(s, name)) for name in FIELDS_IN}


# ---------------------------------------------------------------------------------------------------------------------------
# cameras: the garden demo pose at 1080p.  The scene's centre of mass sits 350 px right of the middle of the frame (CENTRE; for the
# pitch cases 350 px above it, CENTRE_ABOVE): a turn of 1.5 bins then moves it by ~1.62 .. 1.66 bins and a turn of 3 by ~3.19 .. 3.36,
# clear of a rounding tie in either direction - at the middle of the frame a turn of 1.5 bins IS a tie.
# ---------------------------------------------------------------------------------------------------------------------------
W, H = 1920, 1080
_UP, POS, LOOK = (np.asarray(v, dtype=np.float64) for v in camera.DEMO_POSES["garden"])
CENTRE_N = 1000


def _basis():
    fwd = (LOOK - POS) / np.linalg.norm(LOOK - POS)
    right = np.cross(fwd, _UP / np.linalg.norm(_UP))
    right /= np.linalg.norm(right)
    return fwd, right, np.cross(right, fwd)


FWD, RIGHT, UP = _basis()                                  # the still camera's own axes


def _focal(h):
    return 0.5 * h / np.tan(np.radians(camera.THREE_FOV_DEG) / 2.0)           # focal length in pixels


def _at_window_offset(ox, oy):
    return POS + np.linalg.norm(LOOK - POS) * (FWD + RIGHT * (ox / _focal(H)) + UP * (oy / _focal(H)))


CENTRE, CENTRE_ABOVE = _at_window_offset(350.0, 0.0), _at_window_offset(0.0, 350.0)


def centre_sum(c):
    return [float(x) * CENTRE_N for x in c]


def _rot(v, axis, a):
    return v * np.cos(a) + np.cross(axis, v) * np.sin(a) + axis * np.dot(axis, v) * (1.0 - np.cos(a))


def cam_still(w=W, h=H):
    return camera.PerspectiveCamera(w, h, tuple(POS), tuple(LOOK), tuple(UP))


def cam_turned(yaw_bins, pitch_bins, w=W, h=H):
    """Turned about its own position by this many 32-px bins at the middle of the frame: yaw about its up, pitch about its right
    axis (no roll).  A positive yaw moves the picture to the right, a positive pitch moves it down."""
    a, b = np.arctan(yaw_bins * 32.0 / _focal(h)), np.arctan(pitch_bins * 32.0 / _focal(h))
    return camera.PerspectiveCamera(w, h, tuple(POS), tuple(POS + 4.0 * _rot(_rot(FWD, UP, a), RIGHT, b)), tuple(_rot(_rot(UP, UP, a), RIGHT, b)))


def cam_orbited(degrees, w=W, h=H):
    """The whole camera carried about the scene's centre of mass (axis: up): the centre keeps its place on screen, the rest moves."""
    a = np.radians(degrees)
    return camera.PerspectiveCamera(w, h, tuple(CENTRE + _rot(POS - CENTRE, UP, a)), tuple(CENTRE + _rot(LOOK - CENTRE, UP, a)),
                                    tuple(_rot(UP, UP, a)))


def make_inputs(was=None, now=None, **over):
    """A 1080p fp32 draw of 100 000 splats after a draw of the camera `was` (default: the still camera), 128-px list bins, no
    verdict in the mapped words; `over` replaces fields."""
    was = cam_still() if was is None else was
    now = was if now is None else now
    w, h = now.width, now.height
    bins_x, rows = (w + 31) // 32, (h + 31) // 32
    i = {name: 0 for name in FIELDS_IN}
    i.update(centre_sum=centre_sum(CENTRE), centre_n=CENTRE_N, mirror=[0] * MIRROR_WORDS,
             stats_valid=1, stats_bins=((was.width + 31) // 32) * ((was.height + 31) // 32), stats_row_begin=0, stats_width_px=was.width,
             stats_mode=0, stats_view=list(was.model_view()), stats_proj=list(was.projection), stats_width=float(was.width),
             stats_height=float(was.height), stats_count=100000, stats_list_shift=3,
             view=list(now.model_view()), proj=list(now.projection), width=float(w), height=float(h), count=100000, list_shift=3,
             bins_x=bins_x, bin_row_begin=0, bin_row_end=rows, block_cull=1, draw_mode=0, draw_serial=1, no_deep=0,
             deep_min=4096, deep_factor=3, order_motion=0.045, cu_count=256, occupancy=6, list_current=3)
    for k, v in over.items():
        assert k in i, k
        i[k] = v
    return from_struct(to_struct(i))                       # (fp32 fields as the library holds them)


def mirror(serial=5, overflow=0, entries=0, candidates=0, share=0, visible=0, tiles16=0):
    m = [0] * MIRROR_WORDS
    m[0:4] = [serial, overflow, entries & 0xFFFFFFFF, entries >> 32]
    m[4:6] = [candidates, share]
    m[8:12] = [serial, visible, tiles16 & 0xFFFFFFFF, tiles16 >> 32]
    return m


def _nan_view(cam):
    v = list(cam.model_view())
    v[5] = float("nan")
    return v


def _singular_view(cam):
    v = list(cam.model_view())
    v[0:3] = v[4:7]                                        # two equal columns
    return v


def cases():
    """[(name, inputs, expectations on the outputs)]"""
    still, out = cam_still(), []

    def add(name, expect=None, **kw):
        out.append((name, make_inputs(**kw), expect or {}))

    taken = {"order_ok": 1, "same_view": 1, "order_wg": 1, "order_taken": 1}
    refused = {"order_ok": 1, "same_view": 0, "order_taken": 0, "sx": 0, "sy": 0}
    add("same view", dict(taken, sx=0, sy=0))
    add("first draw: no statistics", {"order_ok": 0, "order_wg": 0, "order_taken": 0}, stats_valid=0, stats_bins=0)
    p = list(still.projection)
    p[0] *= 1.5
    add("another proj", refused, now=cam_turned(3, 0), proj=p)
    add("another size", {"order_ok": 0, "order_taken": 0}, now=cam_still(1280, 720))
    add("another height only", refused, now=cam_turned(3, 0), height=1081.0)
    add("another count", refused, now=cam_turned(3, 0), count=99999)
    add("another list shift", refused, now=cam_turned(3, 0), list_shift=4)
    for yaw, pitch in [(1.5, 0), (-1.5, 0), (3, 0), (-3, 0), (0, 1.5), (0, -1.5), (0, 3), (0, -3)]:
        for limit in (0.045, 0.001):                       # no parallax: the order is taken at any speed
            add(f"turn ({yaw}, {pitch}) limit {limit}", dict(taken, turn=(yaw, pitch)), now=cam_turned(yaw, pitch), order_motion=limit,
                centre_sum=centre_sum(CENTRE if pitch == 0 else CENTRE_ABOVE))
    for deg in (0.25, 1.0, 6.0, 12.0):
        for limit in (0.045, 0.0, 100.0):
            near = limit == 100.0 or (limit == 0.045 and deg <= 1.0)
            add(f"orbit {deg} deg limit {limit}", {"order_ok": 1, "same_view": int(near), "order_taken": int(near), "sx": 0, "sy": 0},
                now=cam_orbited(deg), order_motion=limit)
    add("no stat shift, a turn of 0.8 bins", dict(taken, sx=0, sy=0), now=cam_turned(0.8, 0), no_stat_shift=1)
    add("no stat shift, a turn of 3 bins: the whole motion counts", refused, now=cam_turned(3, 0), no_stat_shift=1)
    add("stale order on a moved camera", {"same_view": 0, "order_wg": 1, "order_taken": 1}, now=cam_orbited(12.0), blend_order_stale=1)
    add("no blend order", {"order_ok": 0, "order_wg": 0, "order_taken": 0, "deep_pass": 0}, no_blend_order=1, mirror=mirror(candidates=100))
    add("deep pass keeps the order on motion", {"same_view": 0, "deep_pass": 1, "order_wg": 1, "order_taken": 1},
        now=cam_orbited(12.0), mirror=mirror(candidates=100, share=563))
    add("deep pass, row-major on motion", {"same_view": 0, "deep_pass": 1, "order_wg": 1, "order_taken": 0, "unit_at": 2040, "unit_wgs": 1536},
        now=cam_orbited(12.0), mirror=mirror(candidates=100, share=563), deep_row_major_on_motion=1)
    add("centre behind the camera", refused, now=cam_turned(3, 0), centre_sum=centre_sum(POS - 3.0 * (LOOK - POS)))
    add("no centres", refused, now=cam_turned(3, 0), centre_n=0)
    add("per-scene transforms: no block cull", refused, now=cam_turned(3, 0), block_cull=0)
    add("singular modelView before", {"same_view": 0, "order_taken": 0}, now=cam_turned(3, 0), stats_view=_singular_view(still))
    add("NaN in the view", refused, view=_nan_view(still))
    add("NaN in the view before", refused, now=cam_turned(3, 0), stats_view=_nan_view(still))
    add("more than 8192 bins", {"blend_bins": 32400, "order_ok": 0, "order_wg": 0, "order_taken": 0},
        was=cam_still(7680, 4320), mirror=mirror(candidates=100))
    add("the largest ordered frame", dict(taken, blend_bins=8160), was=cam_still(3840, 2160))
    add("draw mode changed", {"order_ok": 0, "order_taken": 0, "deep_pass": 0}, stats_mode=1, mirror=mirror(candidates=100))
    add("ROP8 after ROP8: an order, no deep pass", dict(taken, deep_pass=0, deep_min=0x7FFFFFFF, unit_wgs=0),
        stats_mode=1, draw_mode=1, mirror=mirror(candidates=100))
    add("another strip", {"order_ok": 0}, bin_row_begin=2, stats_bins=60 * 32)
    for serial in (6, 7, 8):                               # a moving camera runs the schedule job every 8th draw
        add(f"moving camera, draw serial {serial}", {"same_view": 0, "order_wg": int(serial == 7), "order_taken": 0},
            now=cam_orbited(12.0), draw_serial=serial)
    add("32-px list bins keep the job on motion", {"same_view": 0, "order_wg": 1, "order_taken": 0},
        now=cam_orbited(12.0), list_shift=1, stats_list_shift=1)
    add("deep pass by candidates", dict(taken, deep_pass=1), mirror=mirror(candidates=1))
    add("no candidates: no deep pass", dict(taken, deep_pass=0, unit_wgs=0, unit_at=2040), mirror=mirror(candidates=0, share=563))
    add("no_deep", dict(taken, deep_pass=0), mirror=mirror(candidates=100), no_deep=1)
    # unit placement at 256 CUs, occupancy 6
    for cand in (0, 100, 600):
        for share in (0, 563, 1024):
            e = {"deep_pass": int(cand > 0)}
            if cand:
                e.update(unit_at=min(cand, 512) + 384, unit_wgs={0: 512, 563: 512, 1024: 922}[share])
            add(f"units: candidates {cand} share {share}", e, mirror=mirror(candidates=cand, share=share))
    add("units: share word beyond 1024", {"unit_wgs": 922}, mirror=mirror(candidates=100, share=5000))
    add("units last", {"deep_pass": 1, "unit_at": 2040, "unit_wgs": 1536}, mirror=mirror(candidates=100, share=563), deep_units_last=1)
    small = cam_still(320, 200)
    add("units: fewer bins than unit_at", {"blend_bins": 70, "deep_pass": 1, "unit_at": 70, "unit_wgs": 512},
        was=small, mirror=mirror(candidates=100, share=563))
    # the mapped words
    add("feedback: nothing yet", {"view_valid": 0, "serial": 0, "overflow": 0}, mirror=[0] * MIRROR_WORDS)
    add("feedback: an overflow", {"entries_valid": 1, "serial": 9, "overflow": 1, "entries": (3 << 32) | 7, "view_valid": 1, "view_serial": 9,
                                  "visible": 12345, "tiles16": (1 << 32) | 99},
        mirror=mirror(serial=9, overflow=1, entries=(3 << 32) | 7, visible=12345, tiles16=(1 << 32) | 99))
    # entry room
    for need in (0, 2 ** 31, 2 ** 63 - 1, 2 ** 63 + 12345):
        add(f"entry room for {need}", {"room": need + need // 8 + 1024}, need=need)
    # block test
    for share in (None, 0.3, 0.7, 0.95):
        for strip in (0, 1):
            for sw in ({}, {"no_block_list": 1}, {"block_test_always": 1}, {"block_cull": 0}):
                mv, mc = (0, 0) if share is None else (int(share * 200000), 200000)
                add(f"block test: share {share} strip {strip} {sw}", None, measured_visible=mv, measured_count=mc, strip=strip, **sw)
    return out


# tiles per visible splat, walking up and down across every threshold (up at 3.24 / 22.68 / 86.4, down below 2.76 / 19.32 / 73.6)
HYSTERESIS_WALK = [2.0, 2.9, 3.1, 3.3, 3.1, 2.9, 2.7, 5.0, 20.0, 22.0, 23.0, 22.0, 20.0, 19.0, 50.0, 79.0, 85.0, 88.0, 85.0, 75.0, 72.0,
                   10.0, 1.0, 100.0, 2.0, 22.0, 0.5]
HYSTERESIS_VISIBLE = 100000


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "dump", __doc__
    with open(sys.argv[2], "wb") as fh:
        for _, inputs, _ in cases():
            ref.draw_plan(inputs)                          # (the model's own check of the case)
            fh.write(bytes(to_struct(inputs)))
