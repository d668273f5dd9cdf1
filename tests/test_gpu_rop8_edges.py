"""-m gpu: the two shapes of k_tile_blend_rop8 (GS_DRAW_ROP8, GS_DRAW_ROP8_FULL) and k_rop8_window held to an interval model of each
list (tests/rop8_ref.py) on designed scenes (tests/rop8_cases.py) that put list lengths, survivor counts and stop counts on the
edges of the kernel's batch / group / stop logic.  tests/test_rop8_ref.py proves on the CPU that a dropped, repeated, swapped or
reordered survivor at a batch or group edge, a wrong stop count, a wrong start colour, an unrounded alpha and a re-admitted hidden
fragment each fail the comparisons used here.  tests/test_gpu_rop8_mode.py and tests/test_gpu_crops.py hold the mode to the
ROP-emulating oracle statistically on random scenes; this file checks EVERY pixel of every live quadrant on the edges.

Per case and mode, from the draw's own intermediates (gs_mesh_debug_read what = 2 / 8 / 0 / 1 / 9):
  -  the draw is the case: list lengths, survivor counts and, in the bounded mode, the designed stop counts - one candidate each;
  -  every pixel of every live quadrant inside its interval, every other pixel the target's start value; >= 95 % of the checked
     values pinned to one byte, within 0.002 of the share the same case has on the CPU (alpha included: the bounded mode's alpha
     is held to ITS model, the first k survivors);
  -  per bin the pairs composited and the entries scanned (what = 4) equal the predictions;
  -  two more draws of the mode (the blend schedule now orders the bins) give the same bytes;
  -  full walk: gs_mesh_debug_rop8 over the targeted bins lies inside the same interval (its unfused arithmetic's PAD)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rop8_cases as cases
import rop8_ref as rr
from gaussiansplats3d_amd import Context

pytestmark = pytest.mark.gpu
MODES = [rr.FULL, rr.BOUNDED]
PINNED = 0.95
SHARE_MARGIN = 0.002      # the device's records and the CPU oracle's differ in their last bits: a value in 500 may open or close
_cpu_share = {}


def targeted_share(M, c):
    """The pinned share over the live quadrants of the case's targeted bins."""
    ms = [m for (bx, by, _), m in M.items() if (bx, by) in c.targets]
    return sum(int(m.pinned().sum()) for m in ms) / max(sum(m.lo.size for m in ms), 1)


def targeted_models(d, c, mode, rgba, **kw):
    smap = d.splat_of_slot()
    M = {(bx, by, q): rr.model(d, bx, by, q, mode, rgba, None, smap, **kw) for bx, by in c.targets for q in range(4)}
    return {k: m for k, m in M.items() if m is not None}


def cpu_share(name, mode, with_dest=True, unorm24=False):
    """The pinned share of the targeted bins of the same case and mode on the CPU - the oracle's records, the binner's host model
    (tests/test_rop8_ref.py asserts it per targeted bin) - computed once per variant."""
    key = (name, mode, with_dest, unorm24)
    if key not in _cpu_share:
        c = cases.case(name)
        _cpu_share[key] = targeted_share(targeted_models(cases.cpu_draw(c, with_dest=with_dest, unorm24=unorm24), c, mode, c.dest_rgba), c)
    return _cpu_share[key]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def rig_of(ctx):
    rigs = []

    def make(name):
        rigs.append(cases.Rig(ctx, cases.case(name)))
        return rigs[-1]
    yield make
    for r in rigs:
        r.close()


def check(rig, mode, rows=None, rgba=None, what="", cpu=None):
    """One draw in `mode` (the whole frame or the strip `rows`) against the model: (frame, models).  cpu: the pinned share of the
    same frame on the CPU."""
    c = rig.case
    rig.mesh.set_draw_mode(rop8=True, full=mode == rr.FULL)
    frame, st = rig.draw(rows)
    d = rig.draw_of(rows)
    M = rr.models_of(d, mode, rgba, rows)
    row0 = 0 if rows is None else rows[0] * 16
    for (bx, by), per in c.targets.items():                  # the draw really is the case
        if rows is None:
            assert rr.deep_ref.list_of(d, bx, by)[1] == c.list_len[(bx, by)], (what, bx, by)
        for q, t in per.items():
            m = M.get((bx, by, q))
            if m is None:
                assert not rr.deep_ref.live(d, bx, by, q, rows)
                continue
            assert m.S == t.S and m.unique, (what, bx, by, q, m.S, t.S, m.stops)
            if mode == rr.BOUNDED and (bx, by, q) in c.stops:
                assert m.stops == [c.stops[(bx, by, q)]], (what, bx, by, q, m.stops)
    assert all(m.quad.in_band == 0 for m in M.values())
    bad, share, widest = rr.check_frame(frame, M, row0, rgba, what)
    stats = rig.stats(rows)
    bad += rr.check_integers(stats, M, what)
    print(f"{what}: {len(M)} live quadrants, pinned share {share:.4f}, widest interval {widest}, pairs {sum(p for _, p in stats.values())}")
    assert bad == [], bad[:4]
    assert share >= PINNED, (what, share)
    if cpu is not None:                                      # the pinned share is as on the CPU, on the targeted bins
        mine = targeted_share(M, c)
        print(f"{what}: pinned share of the targeted bins {mine:.4f}, on the CPU {cpu:.4f}")
        assert abs(mine - cpu) <= SHARE_MARGIN, (what, mine, cpu)
    assert int(st.splats_walked) == sum(p for _, p in stats.values())
    for _ in range(2):
        np.testing.assert_array_equal(rig.draw(rows)[0], frame)
    return frame, M


def window_check(rig, rgba=None, what=""):
    """gs_mesh_debug_rop8 over every targeted bin of the last (full-frame) draw, inside the full walk's interval."""
    c = rig.case
    d = rig.draw_of()
    M = targeted_models(d, c, rr.FULL, rgba, pad=rr.PAD_UNFUSED)
    bad = []
    for bx, by in c.targets:
        w, h = min(32, c.w - 32 * bx), min(32, c.h - 32 * by)
        got = rig.mesh.rop8_window(32 * bx, 32 * by, w, h)
        for q in range(4):
            m = M.get((bx, by, q))
            if m is not None:
                bad += rr.compare_values(got[m.quad.py - 32 * by, m.quad.px - 32 * bx].astype(np.float64), m, f"{what} window")[0]
    assert bad == [], bad[:4]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in ("dest", "shared")])
def test_every_pixel_inside_the_interval_and_the_walk_counters_as_predicted(rig_of, name, mode):
    rig = rig_of(name)
    frame, M = check(rig, mode, what=f"{name} {mode}", cpu=cpu_share(name, mode))
    if mode == rr.FULL:
        window_check(rig, what=name)
    c = rig.case
    if name == "lengths":                                    # n = 0: the clear colour (check_frame holds every uncovered pixel to it)
        assert len({(bx, by) for bx, by, _ in M}) == len(cases.LENGTHS) and not frame[96:].any()
    if name == "edge8":                                      # strips: bit-equal to the frame's rows, and inside the model of THEIR rows
        parts = []
        for rows in c.strips:
            f, Ms = check(rig, mode, rows=rows, what=f"{name} {mode} rows {rows}")
            assert len([k for k in Ms if k[:2] == (8, 2)]) == 1      # the cut leaves bin (8, 2) one live quadrant: half its waves idle
            parts.append(f)
        np.testing.assert_array_equal(np.concatenate(parts, axis=0), frame)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", ["colour", "float", "unorm24"])
def test_over_a_destination(rig_of, depth, mode):
    """dest: the colour plane alone (the pixels no splat reaches and those under the thin list start from it), then depth + colour
    with one marker of every targeted edge hidden, in float and GS_DEST_DEPTH_UNORM24."""
    rig = rig_of("dest")
    c = rig.case
    rig.set_destination(None if depth == "colour" else c.dest_depth, depth == "unorm24", c.dest_rgba)
    frame, M = check(rig, mode, rgba=c.dest_rgba, what=f"dest {depth} {mode}",
                     cpu=cpu_share("dest", mode, with_dest=depth != "colour", unorm24=depth == "unorm24"))
    if mode == rr.FULL:
        window_check(rig, rgba=c.dest_rgba, what=f"dest {depth}")
    untouched = np.ones(frame.shape[:2], bool)
    untouched[64:96, 96:128] = False
    np.testing.assert_array_equal(frame[untouched], c.dest_rgba[untouched])
    rig.set_destination()


def test_four_blend_bins_walk_one_list_of_a_64_px_list_bin():
    here = os.path.dirname(os.path.abspath(__file__))
    run = subprocess.run([sys.executable, os.path.join(here, "tools", "rop8_child.py"), "shared"],
                         env=dict(os.environ, GSPLAT_LIST_SHIFT="2"), capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    print(out)
    assert [o["mode"] for o in out] == MODES
    for o in out:
        assert o["list_bin_px"] == 64 and len(o["lists"]) == 1 and o["lists"][0][1] == 1000, o
        assert o["bad"] == [] and all(o["equal"]) and o["pinned"] >= PINNED and abs(o["pinned"] - o["pinned_cpu"]) <= SHARE_MARGIN, o
