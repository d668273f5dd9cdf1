"""-m gpu: the composite once a quadrant is more than one chunk deep, held to the TRUTH - the host model of the header's definition
(tests/deep_ref.py: per pixel the plain fp64 front-to-back composite of the quadrant's kept fragments, a derived per-pixel
tolerance of 0.6 .. 1.4 / 255) on designed scenes (tests/deep_cases.py) that put named survivor counts on both sides of the
chunk edges, with markers a dropped, repeated or swapped survivor moves by tens of 1/255.  tests/test_deep_ref.py proves on the CPU
that every such mistake fails the comparison used here.  tests/test_gpu_deep.py and tests/test_gpu_depth.py check that the two
executors AGREE on random piles; this file checks that they are RIGHT at the edges: the chunk table's boundaries in bin_body and in
k_deep_plan / deep_unit / k_deep_fold, the unbounded chunk 31, a list of exactly GS_DEEP_LIST_CAP entries, a chunk that starts in the
middle of a window of a range, the queue's carry, quadrants that are not live, a chunk that saturates on its own, a depth
destination, the exhausted pool.

Per case, from the draw's own intermediates (gs_mesh_debug_read what = 2 / 8 / 0 / 1 / 9):
  deep pass off   every pixel within the model's tolerance; per bin the (splat, quadrant) pairs composited (what = 4) = sum of S_q
                  over the live quadrants (bounds where a quadrant saturates: deep_ref.walk_bounds); the chunk partials the
                  per-bin kernel closed (what = 5) = sum of (chunks - 1), + 1 for every quadrant whose list ends exactly on an edge
                  if the kernel closes there - either is the same composite; the convention must be the same everywhere;
  deep pass on    three draws; the members (what = 5) are the bins the schedule's rule (blend_schedule_ref) picks from the pairs
                  just verified, and they are the bins the case names; bit-equal to the frame above; the pairs again; the closed
                  partials fall by exactly the members' share.
The number of units in the deep pass's plan (sum of chunks over the members' live quadrants) is exposed by no debug read and is
not checked.

What the header promises about the statistics: `splats_walked` and what = 4 count "(splat, 16x16-px quadrant) pairs the blend
evaluated / composited" - for a quadrant no chunk of which saturates that is S_q for either executor.  Where a chunk saturates the
per-bin kernel stops for good and the deep pass walks the chunks behind it as well (the header says the choice of executor is
scheduling only, not that the counts agree): bounds, derived in deep_ref.walk_bounds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_cases as cases
import deep_ref as dr
from gaussiansplats3d_amd import Context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def bins_of(info, c, rows=None):
    """The deep pass's bins as (bx, by) of the frame (what = 5 numbers the bins of the drawn strip, row-major from its first bin row)."""
    cols, b0 = (c.w + 31) // 32, 0 if rows is None else (rows[0] * 16) // 32
    return {(int(b) % cols, int(b) // cols + b0) for b in info["bins"]}


def closed_convention(closed, Q, bins, what):
    """The closed partials of one draw against the model: exact, or - with quadrants whose list ends exactly on an edge among
    `bins` - one of the two counts that treat ALL of them alike.  Returns which ("closes" / "leaves open"; None: no such quadrant)."""
    low, high, on_edge = cases.closed_share(Q, bins)
    assert closed in (low, high), f"{what}: {closed} chunk partials closed, the model says {low} or {high}"
    return None if not on_edge else "closes" if closed == high else "leaves open"


@pytest.fixture
def run_case(ctx):
    """run_case(name, dest=None, unorm24=False) -> (rig, quadrants, frame, figures): the checks of the module's docstring.  The
    rigs' meshes are disposed of when the test is over, however it ends."""
    rigs = []

    def run(name, dest=None, unorm24=False):
        rigs.append(cases.Rig(ctx, cases.case(name)))
        return _run_case(rigs[-1], name, dest, unorm24)
    yield run
    for r in rigs:
        r.close()


def _run_case(rig, name, dest, unorm24):
    c = rig.case
    if dest is not None:
        rig.set_destination(dest, unorm24)
    # deep pass off
    rig.mesh.set_deep_pass(False)
    plain, st0 = rig.draw()
    info0 = rig.mesh.deep_pass_info()
    draw, Q = rig.quads()
    for (bx, by), per in c.targets.items():                  # the draw really is the case: survivor counts and list lengths
        assert dr.list_of(draw, bx, by)[1] == c.list_len[(bx, by)]
        for q, t in per.items():
            assert Q[(bx, by, q)].S == t.S, (name, bx, by, q, Q[(bx, by, q)].S, t.S)
            assert Q[(bx, by, q)].non_saturating() == (not t.saturating)
    assert all(m.in_band == 0 for m in Q.values())
    if dest is not None:                                     # the depths the kernel compared are the model's
        zk = rig.mesh.debug_depths().astype(np.float64)
        want = np.floor(draw.z * 16777215.0 + 0.5) if unorm24 else draw.z
        assert np.abs(zk - want)[draw.vis].max() <= (2.0 if unorm24 else dr.DEPTH_TOL)
    bad, worst, tol = cases.check_frame(plain, Q, c.w, what=f"{name} deep pass off")
    pairs_off = rig.pairs()
    bad += cases.check_pairs(pairs_off, Q, what=f"{name} deep pass off")
    assert bad == [], bad[:4]
    assert len(info0["bins"]) == 0 and not info0["pool_exhausted"] and (int(st0.flags) & 1) == 0
    assert int(st0.splats_walked) == sum(pairs_off.values())
    convention = closed_convention(info0["chunks_closed_by_bins"], Q, None, f"{name} deep pass off")
    # deep pass on
    rig.mesh.set_deep_pass(True)
    frames = [rig.draw() for _ in range(3)]
    info = rig.mesh.deep_pass_info()
    members = bins_of(info, c)
    sched = rig.mesh.blend_schedule()
    assert members == cases.expected_members(pairs_off, c, sched["deep_min"], sched["deep_factor"]), (members, info)
    assert members == set(c.targets), (members, sorted(c.targets))
    for f, _ in frames:
        np.testing.assert_array_equal(f, plain)
    taken = {b for b in members if c.list_len[b] <= dr.LIST_CAP}          # a longer list stays with the per-bin kernel
    bad = cases.check_pairs(rig.pairs(), Q, taken, what=f"{name} deep pass on")
    assert bad == [], bad[:4]
    assert not info["pool_exhausted"]
    kept = {(bx, by) for bx, by, _ in Q} - taken            # the per-bin kernel still closes these bins' chunks, and only these
    assert closed_convention(info["chunks_closed_by_bins"], Q, kept, f"{name} deep pass on") in (None, convention)
    out = dict(case=name, splats=c.scene.count, worst=round(worst, 3), tolerance=round(tol, 3), pairs=sum(pairs_off.values()),
               closed_off=info0["chunks_closed_by_bins"], closed_on=info["chunks_closed_by_bins"], members=sorted(members),
               convention=convention)
    return rig, Q, plain, out


@pytest.mark.parametrize("name", ["ladder_a", "ladder_b", "ladder_c", "tail", "sparse", "saturating"])
def test_both_executors_hold_the_model_at_the_chunk_edges(run_case, name):
    rig, Q, plain, out = run_case(name)
    print(out)
    if name == "ladder_c":                                   # a live quadrant without survivors: no chunk, the clear value
        m = Q[(3, 2, 3)]
        assert m.S == 0 and not plain[m.py, m.px].any()
    if name == "saturating":                                 # nothing behind the stack shows: its pixels are the stack's white
        m = Q[(3, 2, 0)]
        assert (plain[m.py, m.px, 3] == 255).all()


def test_a_list_that_ends_on_a_chunk_edge_is_treated_the_same_way_in_every_case(run_case):
    """1024 (ladder_a), 2048 and 4096 (ladder_b), 5120 (ladder_c): the per-bin kernel closes the chunk such a list fills, or leaves
    it open - one way for all (within a draw closed_convention() holds it; here across the cases)."""
    seen = set()
    for name in ("ladder_a", "ladder_b", "ladder_c"):
        rig, Q, plain, out = run_case(name)
        assert out["convention"] is not None
        seen.add(out["convention"])
    print(seen)
    assert len(seen) == 1, seen


def test_a_list_of_exactly_the_cap_is_a_member_and_one_more_entry_is_not(run_case):
    """cap: bin (1, 1) holds GS_DEEP_LIST_CAP entries - 64 full ranges - and is composited by the deep pass; bin (6, 3) holds one
    more, is named by the selection and stays with the per-bin kernel: the closed partials fall by exactly the first bin's share
    and keep the second's (run_case asserts it from the lists' lengths)."""
    rig, Q, plain, out = run_case("cap")
    print(out)
    share = {b: cases.closed_share(Q, {b}) for b in ((1, 1), (6, 3))}
    assert share[(6, 3)][2] == [] and out["closed_on"] == share[(6, 3)][0] > 0
    assert out["closed_off"] - out["closed_on"] in (share[(1, 1)][0], share[(1, 1)][1])


def test_quadrants_that_are_not_live_and_strips_that_cut_the_deep_bin(run_case):
    """edge: the deep bins are the last column of a frame that is 16 mod 32 both ways.  The strips' frames concatenate to the full
    frame bit for bit, with the deep pass off and on, and each strip is held to the model of ITS OWN rows and lists."""
    rig, Q, plain, out = run_case("edge")
    print(out)
    c = cases.case("edge")
    assert sorted(Q) == [(8, 2, 0), (8, 2, 2), (8, 5, 0)]
    strips = []
    for rows in c.strips:
        rig.mesh.set_deep_pass(False)
        f0, _ = rig.draw(rows)
        _, Qs = rig.quads(rows)
        pairs0 = rig.pairs(rows)
        bad, worst, tol = cases.check_frame(f0, Qs, c.w, row0=rows[0] * 16, what=f"edge rows {rows}")
        bad += cases.check_pairs(pairs0, Qs, what=f"edge rows {rows} deep pass off")
        rig.mesh.set_deep_pass(True)
        for _ in range(3):                                   # every strip warms its own statistics up to its own deep pass
            f, _ = rig.draw(rows)
            np.testing.assert_array_equal(f, f0)
        members = bins_of(rig.mesh.deep_pass_info(), c, rows)
        assert members == cases.expected_members(pairs0, c, rows=rows) and (8, 2) in members, (rows, members)
        assert len([k for k in Qs if k[:2] == (8, 2)]) == 1  # the cut leaves bin (8, 2) ONE live quadrant in either strip
        bad += cases.check_pairs(rig.pairs(rows), Qs, members, what=f"edge rows {rows} deep pass on")
        assert bad == [], bad[:4]
        strips.append(f0)
    np.testing.assert_array_equal(np.concatenate(strips, axis=0), plain)


@pytest.mark.parametrize("unorm24", [False, True], ids=["float", "unorm24"])
def test_both_executors_under_a_depth_destination(run_case, unorm24):
    """depth: ladder_b with every third survivor and one marker of each edge pair behind the destination's plane on the right half
    of every quadrant.  Hidden survivors count towards the chunk edges in both executors."""
    c = cases.case("depth")
    rig, Q, plain, out = run_case("depth", dest=c.dest_depth, unorm24=unorm24)
    print(out)
    rig.set_destination(None)
    bare, _ = rig.draw()
    for (bx, by), per in c.targets.items():                  # the plane shows AT the marker pixels: a marker of every edge pair is hidden
        for q in per:
            m = Q[(bx, by, q)]
            marks = cases.marker_pixels(c, m) & ((m.px % 16) >= 8)
            d = np.abs(bare[m.py, m.px].astype(np.int32) - plain[m.py, m.px].astype(np.int32)).max(axis=1)
            assert d[marks].max() >= 8, (bx, by, q, int(d[marks].max()))


def child(what, names, env):
    here = os.path.dirname(os.path.abspath(__file__))
    run = subprocess.run([sys.executable, os.path.join(here, "tools", "deep_child.py"), what, names], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    print(out)
    return out


def test_an_exhausted_pool_still_composites_the_truth():
    """GSPLAT_POOL_SLOTS=2 on ladder_b and tail, the deep pass off: the draw says so and every pixel is still within the model's
    tolerance, the stop rule's term taken for ONE long chunk (0.57 / 255 + the ambiguous fragments)."""
    for o in child("pool", "ladder_b,tail", {"GSPLAT_POOL_SLOTS": "2"}):
        assert o["pool_exhausted"] and (o["flags"] & 1) == 1 and o["closed"] >= 2, o
        assert o["bad"] == [] and o["worst"] <= 1.0, o


def test_the_deep_pass_on_quadrants_of_one_and_two_chunks():
    """GSPLAT_DEEP_MIN=256 GSPLAT_DEEP_FACTOR=1 on ladder_a (1023 / 1024 / 1025 / 1281 survivors)."""
    (o,) = child("deep", "ladder_a", {"GSPLAT_DEEP_MIN": "256", "GSPLAT_DEEP_FACTOR": "1"})
    assert o["deep_min"] == 256 and o["deep_factor"] == 1
    assert o["bins"] == o["want"] == [[3, 2]], o
    assert all(o["equal"]) and o["bad"] == [] and o["worst"] <= 1.0 and o["closed"] == 0, o
