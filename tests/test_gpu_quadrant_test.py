"""-m gpu: the blend's quadrant test (csrc/tile_blend.hip: quadrant_mask + exact_quadrants) held to the per-pixel fragment rule at
every site that evaluates it - the per-bin blend, k_deep_scan for the deep units, k_tile_blend_rop8 in both ROP8 draw modes and
k_surface - on the scenes of quadrant_cases.py, judged by the host model (quadrant_ref.py) from the draw's OWN records and rects
(gs_mesh_debug_read what = 0 / 1 / 3), as tests/test_gpu_bin_lists.py judges the lists.  k_rop8_window is held to the same rule: it
does not call the test (it applies the fragment rule per pixel from the rect alone), so it is the device's own witness of it.

Every hand-made splat is drawn alone (a render list of one index into the case's mesh), opaque and white, so that a quadrant dropped
wrongly is a hole nothing else fills.  Every pixel of every draw is judged: drawn (alpha >= 4: an opaque fragment at the cut
contributes 4.67 / 255) where fp64 says a fragment is inside the cut by more than the band, exactly clear where every fragment is
outside it by more than the band or the rect does not cover the tile; only the pixels inside the band are exempt, and each test
prints how many that was.  The (splat, quadrant) pairs a draw walks (gs_mesh_debug_read what = 4) are held between the model's
must-keep pairs and must-keep + free pairs, bin by bin: the only check of how many quadrants the test keeps, which is the blend's cost."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quadrant_cases as cases
import quadrant_ref as qr
import surface_cases
import surface_ref
from gaussiansplats3d_amd import Context, SplatMesh
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
NONE = surface_ref.NONE
HAND = ["needle_diag", "corner_graze", "axis_aligned", "inside"]
STRIPS = [(0, 1), (6, 7), (1, 6)]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    _rigs.clear()
    c.close()                                               # (with the rigs' meshes)


class Rig:
    """One mesh per case; a draw is a render list into it.  The vertex stage projects every uploaded splat on every draw, so the
    records, rects and flags of the first draw are those of all of them (same camera): read once, shared, unchanged."""

    def __init__(self, ctx, case, alpha=None):
        s = case.scene
        rgba = s.rgba.copy()
        if alpha is not None:
            rgba[:, 3] = alpha
        self.case = case
        self.mesh = SplatMesh(ctx, s.count, s.sh_degree)
        self.mesh.build(s.centers, s.cov, rgba, s.sh if s.sh_degree else None)
        self.mesh.set_camera(case.cam)
        self.draw(0)
        self.recs, self.rects, self.vis = self.mesh.debug_records()
        self._classes, self._pairs = {}, None

    def indexes(self, k):
        idx = self.case.draws[k]
        return idx if self.case.order is None or len(idx) == 1 else self.case.order

    def draw(self, k, tile_rows=None):
        idx = self.indexes(k)
        self.mesh.update_render_indexes(idx, len(idx))
        return self.mesh.render(tile_rows=tile_rows)[0]

    def classes(self, k):
        if k not in self._classes:
            idx = self.case.draws[k]
            self._classes[k] = qr.pixel_classes(self.recs, self.rects, idx[self.vis[idx]], self.case.w, self.case.h)
        return self._classes[k]

    def pairs(self):
        if self._pairs is None:
            self._pairs = qr.analyse(self.recs, self.rects, self.vis, self.case.w, self.case.h)
        return self._pairs


_rigs = {}


def rig_of(ctx, case, alpha=None):
    key = (case.name, alpha)
    if key not in _rigs:
        _rigs[key] = Rig(ctx, case, alpha)
    return _rigs[key]


def coverage_complaints(frame, sure, none, outside, what):
    """The coverage rule on one RGBA8 frame / window; returns (complaints, exempt pixels)."""
    bad = []
    if outside.any():
        bad.append(f"{what}: {int(outside.sum())} pixels inside the cut lie outside the splat's own rect")
    hole = sure & (frame[..., 3] < 4)
    if hole.any():
        y, x = (int(v[0]) for v in np.nonzero(hole))
        bad.append(f"{what}: {int(hole.sum())} pixels a fragment certainly covers are not drawn, first ({x}, {y}) alpha {int(frame[y, x, 3])}")
    stray = none & (frame != 0).any(axis=-1)
    if stray.any():
        y, x = (int(v[0]) for v in np.nonzero(stray))
        bad.append(f"{what}: {int(stray.sum())} pixels no fragment reaches are not clear, first ({x}, {y}) = {frame[y, x].tolist()}")
    return bad, int((~sure & ~none).sum())


def report(name, bad, exempt, judged, draws):
    print(f"{name}: {draws} draws, {judged} pixels judged, {exempt} exempt (inside the band of {qr.BAND:.1e})")
    assert bad == [], f"{len(bad)} complaints, first: {bad[:3]}"


# -- coverage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", HAND)
def test_fp32_draw_window_and_surface_cover_exactly_what_the_fragment_rule_keeps(ctx, family):
    """The per-bin blend, k_rop8_window over the whole frame (blocks of at most 65536 px) and k_surface at 0.99: an opaque
    fragment takes T to at most 1 - exp(-4) = 0.982, so every kept fragment is the surface and every pixel without one has none."""
    bad, exempt, judged, draws = [], 0, 0, 0
    for case in cases.family(family):
        rig = rig_of(ctx, case)
        w, h = case.w, case.h
        blocks = [(x0, min(x0 + 65536 // h, w)) for x0 in range(0, w, 65536 // h)]
        for k in range(len(case.draws)):
            sure, none, outside = rig.classes(k)
            frame = rig.draw(k)
            assert frame.shape == (h, w, 4)
            b, e = coverage_complaints(frame, sure, none, outside, f"{case.name} draw {k} fp32")
            bad += b
            win = np.concatenate([rig.mesh.rop8_window(x0, 0, x1 - x0, h) for x0, x1 in blocks], axis=1)
            bad += coverage_complaints(win, sure, none, outside, f"{case.name} draw {k} rop8 window")[0]
            ids, depth = rig.mesh.surface(0, 0, w, h, 0.99)
            splat = int(case.draws[k][0])
            wrong = (sure & (ids != splat)) | (none & (ids != NONE)) | ((ids != NONE) & (ids != splat))
            if wrong.any():
                y, x = (int(v[0]) for v in np.nonzero(wrong))
                bad.append(f"{case.name} draw {k} surface: {int(wrong.sum())} pixels, first ({x}, {y}) answers {int(ids[y, x])}, sure {bool(sure[y, x])}, none {bool(none[y, x])}")
            exempt += e
            judged += h * w
            draws += 1
        # two draws per case through the surface model as well, the band as its eta: depth and the list walk included
        for k in (0, len(case.draws) - 1):
            rig.draw(k)
            x0 = max(0, w - 160)                            # (the model walks pixel by pixel in Python: the frame's last 160 columns)
            ids, depth = rig.mesh.surface(x0, 0, w - x0, h, 0.99)
            model = surface_cases.draw_of(rig.mesh, case.scene.centers)
            bad += surface_ref.check_window(model, x0, 0, ids, depth, 0.99, eta=qr.BAND)[:3]
    report(family, bad, exempt, judged, draws)


@pytest.mark.parametrize("full", [True, False], ids=["rop8_full", "rop8"])
@pytest.mark.parametrize("family", HAND)
def test_rop8_draws_cover_exactly_what_the_fragment_rule_keeps(ctx, family, full):
    """GS_DRAW_ROP8_FULL (one pass to the list's end) and GS_DRAW_ROP8 (both passes)."""
    bad, exempt, judged, draws = [], 0, 0, 0
    for case in cases.family(family):
        rig = rig_of(ctx, case)
        rig.mesh.set_draw_mode(rop8=True, full=full)
        try:
            for k in range(len(case.draws)):
                b, e = coverage_complaints(rig.draw(k), *rig.classes(k), f"{case.name} draw {k}")
                bad += b
                exempt += e
                judged += case.h * case.w
                draws += 1
        finally:
            rig.mesh.set_draw_mode(rop8=False)
    report(family, bad, exempt, judged, draws)


# -- pair counts ----------------------------------------------------------------------------------------------------------------------
def sandwich(pairs, sel, walked, bin_row_begin, what):
    rows, cols = walked.shape
    lo = pairs.per_bin(sel & pairs.must_keep, cols, rows, bin_row_begin)
    hi = lo + pairs.per_bin(sel & pairs.free, cols, rows, bin_row_begin)
    wrong = (walked < lo) | (walked > hi)
    if not wrong.any():
        return []
    y, x = (int(v[0]) for v in np.nonzero(wrong))
    return [f"{what}: {int(wrong.sum())} bins outside [must keep, must keep + free], first bin ({x}, {y + bin_row_begin}): walked "
            f"{int(walked[y, x])}, must keep {int(lo[y, x])}, free {int(hi[y, x] - lo[y, x])}"]


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_pairs_walked_lie_between_the_needed_and_the_allowed_bin_by_bin(ctx, family):
    """GS_DRAW_ROP8_FULL walks every list whole: per bin, #must-keep <= pairs <= #must-keep + #free.  The fp32 draw of the same
    scene with every alpha 1 / 255 (nothing saturates) must walk the same number, bin for bin."""
    bad, total, free = [], 0, 0
    for case in cases.family(family):
        rig, faint = rig_of(ctx, case), rig_of(ctx, case, alpha=1)
        assert np.array_equal(rig.recs[rig.vis][:, :6], faint.recs[faint.vis][:, :6]) and np.array_equal(rig.vis, faint.vis)
        P = rig.pairs()
        rig.mesh.set_draw_mode(rop8=True, full=True)
        try:
            for k, idx in enumerate(case.draws):
                rig.draw(k)
                walked = rig.mesh.blend_bin_stats()[..., 1].astype(np.int64) // 2
                sel = np.isin(P.rec, idx)
                bad += sandwich(P, sel, walked, 0, f"{case.name} draw {k} rop8_full")
                faint.draw(k)
                again = faint.mesh.blend_bin_stats()[..., 1].astype(np.int64) // 2
                if not np.array_equal(again, walked):
                    y, x = (int(v[0]) for v in np.nonzero(again != walked))
                    bad.append(f"{case.name} draw {k}: the faint fp32 draw walked {int(again[y, x])} pairs in bin ({x}, {y}), rop8_full {int(walked[y, x])}")
                total += int(walked.sum())
                free += int((sel & P.free).sum())
        finally:
            rig.mesh.set_draw_mode(rop8=False)
        kept = P.kept_by(rig.recs, rig.rects)
        assert not (P.must_keep & ~kept).any() and not (P.must_drop & kept).any(), "the restatement on the device's own records"
    print(f"{family}: {total} pairs walked, {free} free pairs")
    assert total > 0 and bad == [], f"{len(bad)} complaints, first: {bad[:3]}"


# -- strips ---------------------------------------------------------------------------------------------------------------------------
def strip_stats(mesh, case, rows):
    y0, y1 = qr.live_rows(case.h, rows)
    b0, b1 = y0 // 32, (y1 + 31) // 32
    cols = (case.w + 31) // 32
    out = np.zeros(((b1 - b0) * cols, 2), dtype=np.uint32)
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 4, out.ctypes.data, out.shape[0]))
    return out.reshape(b1 - b0, cols, 2)[..., 1].astype(np.int64) // 2, b0


@pytest.mark.parametrize("family, draws", [("needle_diag", (7, 36)), ("corner_graze", (3, 41))], ids=["needle_diag", "corner_graze"])
def test_single_tile_rows_and_a_cut_reproduce_the_frame_and_walk_their_own_pairs(ctx, family, draws):
    """Tile rows 0 and 6 (the frame's partial top row) alone, and the cut (1, 6): the same bits as the full frame's rows, and the
    pairs walked obey the sandwich with live() restricted to the strip (from the strip draw's own rects)."""
    case = cases.family(family)[0]
    rig = rig_of(ctx, case)
    bad = []
    for k in draws:
        full = rig.draw(k)
        assert full[..., 3].any()
        for rows in STRIPS:
            y0, y1 = qr.live_rows(case.h, rows)
            part = rig.draw(k, tile_rows=rows)
            assert part.shape == (y1 - y0, case.w, 4)
            if not np.array_equal(part, full[y0:y1]):
                bad.append(f"{case.name} draw {k} rows {rows}: {int((part != full[y0:y1]).any(axis=-1).sum())} pixels differ from the full frame")
            walked, b0 = strip_stats(rig.mesh, case, rows)
            recs, rects, vis = rig.mesh.debug_records()
            P = qr.analyse(recs, rects, vis, case.w, case.h, rows=rows, only=case.draws[k])
            bad += sandwich(P, np.ones(P.rec.shape, dtype=bool), walked, b0, f"{case.name} draw {k} rows {rows}")
    rig.draw(0)                                             # (the rig's planes are those of a full-frame draw)
    assert bad == [], bad[:3]


# -- the deep pass --------------------------------------------------------------------------------------------------------------------
DEEP_SCRIPT = """
import json, sys
sys.path[:0] = [{tests!r}, {root!r}]
import numpy as np
import quadrant_cases as cases
import test_gpu_quadrant_test as T
from gaussiansplats3d_amd import Context
c = Context(0)
case = cases.family("needle_diag")[0]
rig = T.Rig(c, case)
out = []
for k in {draws!r}:
    rig.mesh.set_deep_pass(False)
    plain = rig.draw(k)
    rig.mesh.set_deep_pass(True)
    frames = [rig.draw(k) for _ in range(3)]
    info = rig.mesh.deep_pass_info()
    sched = rig.mesh.blend_schedule()
    bad, exempt = T.coverage_complaints(frames[-1], *rig.classes(k), "deep pass draw %d" % k)
    out.append(dict(draw=k, bins=int(len(info["bins"])), deep_min=sched["deep_min"], deep_factor=sched["deep_factor"],
                    equal=[bool(np.array_equal(f, plain)) for f in frames], bad=bad, exempt=exempt, drawn=int((plain[..., 3] > 0).sum())))
print(json.dumps(out))
rig.mesh.dispose(); c.close()
"""


def test_the_deep_pass_takes_one_entry_bins_and_draws_the_same_needle():
    """GSPLAT_DEEP_MIN=1 GSPLAT_DEEP_FACTOR=1 make every walked bin a candidate of the deep pass (k_deep_scan and the deep units).
    The two switches are read once per process, at its first draw, so the draws run in a child process: the third draw of a
    needle runs the pass on a non-empty set of bins, is bit-equal to the draw with set_deep_pass(False) and meets the coverage rule."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GSPLAT_DEEP_MIN="1", GSPLAT_DEEP_FACTOR="1")
    script = DEEP_SCRIPT.format(tests=here, root=os.path.dirname(here), draws=[7, 36])
    run = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    print(out)
    for o in out:
        assert o["deep_min"] == 1 and o["deep_factor"] == 1
        assert o["bins"] > 0, "the schedule picked no bin for the deep pass"
        assert all(o["equal"]) and o["bad"] == [] and o["drawn"] > 100
