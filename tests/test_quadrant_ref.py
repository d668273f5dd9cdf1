"""CPU tier of the quadrant test's tests: the host model (quadrant_ref.py) against itself, the np.float32 restatement of
quadrant_mask + exact_quadrants (csrc/tile_blend.hip) against the per-pixel fragment rule on the oracle's records of every case
(quadrant_cases.py), the mutations that must fail, and the measurements behind the band and the two caps."""
import numpy as np
import pytest

import quadrant_cases as cases
import quadrant_ref as qr
import surface_ref

NAMES = [n for fam in cases.FAMILIES for n in cases.NAMES[fam]]
_pairs = {}


def every_case():
    return [cases.case(n) for n in NAMES]


def planes_and_pairs(case):
    """The oracle's planes of a case and its classed pairs: computed once, shared by every test, never modified."""
    if case.name not in _pairs:
        recs, rects, vis = cases.oracle_planes(case)
        _pairs[case.name] = (recs, rects, vis, qr.analyse(recs, rects, vis, case.w, case.h))
    return _pairs[case.name]


@pytest.fixture(params=NAMES)
def case(request):
    return cases.case(request.param)


def test_the_cases_are_what_they_are_named_for():
    by_name = {c.name: planes_and_pairs(c) for c in every_case()}
    recs, rects, vis, P = by_name["needle_diag_far"]
    cx = surface_ref.rec_fields(recs)[0].astype(np.float64)
    far = P.must_keep & (np.abs(P.tx * 16 + 8 - cx[P.rec]) >= 900)
    assert vis.all() and far.sum() > 100, "quadrants 900 px and more from the centre that the needle does reach"
    assert (P.must_drop & (np.abs(P.tx * 16 + 8 - cx[P.rec]) >= 900)).sum() > 100
    _, _, ax, ay, ex, ey, _ = (v.astype(np.float64) for v in surface_ref.rec_fields(recs))
    assert (np.hypot(ex, ey) / np.hypot(ax, ay)).max() > 500, "aspect ratios beyond 500 : 1"
    # a graze: one pixel of the quadrant passes the rule, by 2e-4 .. 5e-3
    for name in ("needle_diag", "needle_diag_far"):
        P = by_name[name][3]
        assert ((P.foot == 1) & P.must_keep & (P.pmin64 > qr.CUT - 5e-3)).sum() >= 8, name
    recs, rects, vis, P = by_name["corner_graze"]
    assert vis.all() and len(vis) == 80 and (P.must_drop.sum() > 50) and ((P.foot > 0) & (P.foot <= 3)).sum() > 20
    assert (P.tx == 8).any() and (P.ty == 6).any(), "the partial tiles of the right and the top edge"
    for name in ("axis_aligned", "axis_aligned_129x97", "axis_aligned_127x95"):
        recs, rects, vis, P = by_name[name]
        _, _, ax, ay, ex, ey, _ = surface_ref.rec_fields(recs[vis])
        assert ((ax * ay + ex * ey) == 0).any(), f"{name}: a record with m01 == 0"
    for (name, at) in (("axis_aligned_129x97", (64.5, 48.5)), ("axis_aligned_127x95", (63.5, 47.5)), ("inside_129x97", (64.5, 48.5)), ("inside_127x95", (63.5, 47.5))):
        recs = by_name[name][0]
        cx, cy = surface_ref.rec_fields(recs)[:2]
        assert cx[0] == np.float32(at[0]) and cy[0] == np.float32(at[1]), f"{name}: the centre is exactly on a pixel centre"
    box = by_name["inside"][3].boxmin64
    assert by_name["inside"][2].all() and (box == 0).sum() >= 6 and ((box > 0) & (box < 2)).sum() >= 12


def test_what_the_test_does_with_a_nan_record():
    """The vertex stage emits no such record (quadrant_cases.py).  If one arrived: a centre that is NaN in both coordinates keeps every quadrant (no
    bound is formed: qmin = 0); a NaN coefficient keeps the quadrant the centre lies in and the ones tested on two edges, but where only one
    edge faces the centre fminf(NaN, GS_HUGE) is GS_HUGE and the quadrant goes - so `NaN keeps` is not something a caller may
    lean on."""
    f = np.zeros((3, 6), dtype=np.float32)
    f[:] = [10.5, 10.5, 0.3, 0.1, -0.1, 0.3]                 # centre in quadrant 0 of bin (0, 0)
    f[0, :2] = np.nan
    f[1, 5] = np.nan
    f[2, :2] = [1e4, 1e4]                                   # (a finite record far away, to see the test drop at all)
    recs = np.zeros((3, 8), dtype=np.uint32)
    recs[:, :6] = f.view(np.uint32)
    got = qr.exact_quadrants32(recs, 0, 0)
    assert got[0] == 15 and got[2] == 0 and (got[1] & 9) == 9
    assert qr.exact_quadrants32(recs, 3, 1)[0] == 15


def test_box_minimum_is_below_every_pixel_and_agrees_with_dense_sampling(case):
    recs, rects, vis, P = planes_and_pairs(case)
    assert P.rec.size > 0
    assert (P.boxmin64 <= P.pmin64 * (1 + 1e-12) + 1e-12).all()
    assert not (P.must_keep & P.must_drop).any()
    # a handful of pairs: the box on a 241 x 241 grid (1/16 px) - never below the exact minimum, and within the grid's reach of it
    pick = np.unique(np.concatenate([np.argsort(np.abs(P.boxmin64 - qr.CUT))[:4], np.nonzero(P.boxmin64 > 0)[0][:2], [0, P.rec.size - 1]]))
    g = np.arange(241) / 16.0
    for j in pick:
        cx, cy, ax, ay, ex, ey = (float(v[P.rec[j]]) for v in surface_ref.rec_fields(recs)[:6])
        dx = (P.tx[j] * 16 + 0.5 + g)[None, :] - cx
        dy = (P.ty[j] * 16 + 0.5 + g)[:, None] - cy
        dense = ((ax * dx + ay * dy) ** 2 + (ex * dx + ey * dy) ** 2).min()
        grad = 2.0 * np.sqrt(max(dense, 1e-30)) * np.hypot(np.hypot(ax, ay), np.hypot(ex, ey))          # |grad power| <= 2 sqrt(power) |M|
        assert P.boxmin64[j] <= dense * (1 + 1e-12) and dense - P.boxmin64[j] <= grad / 16.0 + 1e-9, (case.name, int(j), dense, P.boxmin64[j])


def test_the_kernel_restatement_drops_nothing_the_pixel_rule_keeps(case):
    recs, rects, vis, P = planes_and_pairs(case)
    kept = P.kept_by(recs, rects)
    print(f"{case.name}: {P.rec.size} rect-mask pairs, {int(P.must_keep.sum())} must keep, {int(P.must_drop.sum())} must drop, "
          f"{int(P.free.sum())} free; the test keeps {int(kept.sum())}")
    assert not (P.must_keep & ~kept).any(), "a quadrant is dropped that fp64 says a pixel needs"
    assert not (P.keep32 & ~kept).any(), "a quadrant is dropped in which the kernel's own fp32 rule keeps a pixel"


def test_the_kernel_restatement_keeps_nothing_it_must_drop(case):
    recs, rects, vis, P = planes_and_pairs(case)
    assert not (P.must_drop & P.kept_by(recs, rects)).any()


@pytest.mark.parametrize("variant", ["expanded", "minimiser_sign", "swap_rcp", "one_edge", "max_not_min"])
def test_a_mutated_test_drops_needed_quadrants(variant):
    """Each wrong version loses must-keep pairs on at least two cases (frames), the expanded form on the needles of both frames of
    needle_diag: beyond a 50 : 1 aspect ratio m00 x^2 + 2 m01 x y + m11 y^2 cancels to nothing.  (Removing the 1.0001 margin is not
    asked to break anything: it does not, on any case.)"""
    lost = {}
    for c in every_case():
        recs, rects, vis, P = planes_and_pairs(c)
        lost[c.name] = int((P.must_keep & ~P.kept_by(recs, rects, variant)).sum())
    print(variant, lost)
    assert sum(1 for v in lost.values() if v > 0) >= 2, lost
    if variant == "expanded":
        assert lost["needle_diag"] > 0 and lost["needle_diag_far"] > 0


def test_the_band_holds_on_the_cases(case):
    """BAND is 4 x the worst |power32 - power64| measured here (quadrant_ref's docstring records the figures), and the two caps: the
    free pairs are at most 2 % of the rect-mask pairs and the pixels within the band of the cut at most 1 % of the footprint."""
    recs, rects, vis, P = planes_and_pairs(case)
    worst = qr.measure_band(recs, rects, vis, case.w, case.h)
    free, near, foot = int(P.free.sum()), int(P.near.sum()), int(P.foot.sum())
    print(f"{case.name}: worst |power32 - power64| = {worst:.3e} (band {qr.BAND:.2e}); free pairs {free} of {P.rec.size} = "
          f"{100.0 * free / P.rec.size:.2f} %; pixels within the band {near} of {foot} = {100.0 * near / foot:.3f} %")
    assert 4.0 * worst <= qr.BAND
    assert free <= 0.02 * P.rec.size
    assert near <= 0.01 * foot


def test_the_band_is_not_wider_than_the_measurement_asks():
    worst = max(qr.measure_band(*cases.oracle_planes(c), c.w, c.h) for c in every_case())
    assert qr.BAND <= 4.0 * worst * 1.02, "BAND is the measurement, rounded to two digits"
    assert 4.0 * worst > surface_ref.ETA and qr.BAND < 2.5 * surface_ref.ETA      # why check_window takes an eta
