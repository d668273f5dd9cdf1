"""Host model (numpy) of the blend's quadrant test (csrc/tile_blend.hip: quadrant_mask + exact_quadrants): which of a 32-px bin's
four 16 x 16 quadrants a list entry is staged for.  The contract is the per-pixel fragment rule `pw < GS_POWER_CUT` of alpha_of:
a quadrant may be dropped only if the rule discards the splat at every one of its pixels.

Inputs are device-style: records uint32 [n, 8], tile rects uint32 [n, 2], the visibility flags and the frame (or strip).  A PAIR is
(record, 16-px tile of its rect); the tile is quadrant (tx & 1) + 2 (ty & 1) of bin (tx >> 1, ty >> 1), and only pairs whose
quadrant is live (BinGeom::live: inside the viewport and the strip's rows) are ever walked.  Per pair the model holds

    pmin64    the smallest fp64 power over the quadrant's pixel centres inside the frame / strip (brute force, <= 256 pixels),
    boxmin64  the exact fp64 minimum of the same convex form over the continuous box of pixel centres [X0, X0 + 15] x [Y0, Y0 + 15]
              (interior, four edges, corners): the quantity the kernel bounds,
    keep32    whether the kernel's own staged fp32 power (surface_ref.power32) passes `pw < CUT` at some pixel of the quadrant,

and classes it   must keep  pmin64 < CUT - BAND,   must drop  boxmin64 > LIMIT + BAND,   free  otherwise
(LIMIT = GS_POWER_CUT * 1.0001f + 1e-6f, what the kernel compares its edge minimum with).  boxmin64 <= pmin64, so no pair is both.

BAND is measured, not chosen (tests/test_quadrant_ref.py::test_the_band_holds_on_the_cases prints the figures and re-asserts
them): the worst |power32 - power64| over every (visible record of the oracle's vertex stage, pixel with power64 < CUT + 1) of the
cases of quadrant_cases.py, every bin the record's rect reaches included, however far the record's centre is from it:
    needle_diag 4.934e-5 (136 x 104) / 2.357e-5 (1056 x 72)   corner_graze 6.89e-6   axis_aligned 5.34e-6   inside 1.773e-5
    random_small 1.905e-5 (seed 5) / 2.523e-5 (seed 6)
    worst 4.934e-5   ->   BAND = 4 x = 2.0e-4  (3.5e-5 of the cut)
4 x is the margin surface_ref gave its ETA for the same reason: device records differ from the oracle's in the last bits.  (A needle
1000 px from a bin does not cost more: near its contour the only large products are along its axis, where the coefficients are
K / 1024.)  The figure is twice surface_ref.ETA / 4, so surface_ref.check_window takes the band as its `eta` where these scenes are
judged by it.
"""
from dataclasses import dataclass

import numpy as np

import surface_ref as ref

TILE, BIN = ref.TILE, ref.BIN
CUT = ref.CUT
CUT32 = np.float32(5.7707801636)
LIMIT32 = np.float32(np.float32(CUT32 * np.float32(1.0001)) + np.float32(1e-6))        # folded in fp32, as the compiler folds it
LIMIT = float(LIMIT32)
HUGE32 = np.float32(1.2676506e30)
BAND = 2.0e-4
VARIANTS = ("kernel", "expanded", "minimiser_sign", "swap_rcp", "one_edge", "max_not_min", "no_margin")


def rect_fields(rects):
    r = np.asarray(rects, dtype=np.uint32).reshape(-1, 2)
    return (r[:, 0] & 0xFFFF).astype(np.int64), (r[:, 0] >> 16).astype(np.int64), (r[:, 1] & 0xFFFF).astype(np.int64), (r[:, 1] >> 16).astype(np.int64)


# -- fp64: what is true -------------------------------------------------------------------------------------------------------------
def pixel_power64(recs, px, py):
    """fp64 power of records [m] at the pixel centres (px, py) [p] (the pixels of ONE quadrant that lie inside the frame): the whole
    table float64 [m, p] and its minimum per record (inf where p = 0)."""
    pw = ref.power64(recs, px, py)
    return pw, (pw.min(axis=1) if pw.shape[1] else np.full(pw.shape[0], np.inf))


def _form64(recs):
    cx, cy, ax, ay, ex, ey, _ = (np.asarray(v, np.float64) for v in ref.rec_fields(recs))
    return cx, cy, ax, ay, ex, ey


def box_min64(recs, x0, y0):
    """Exact fp64 minimum of (a.d)^2 + (b.d)^2 over d = p - centre, p in the box of pixel centres [x0 + 0.5, x0 + 15.5] x
    [y0 + 0.5, y0 + 15.5] (x0, y0: the quadrant's first pixel, one per record).  The form is convex with its minimum 0 at d = 0: 0
    when the centre lies in the box, else the least of the four edges' 1-D minima (clamped to the edge, so the corners are in)."""
    cx, cy, ax, ay, ex, ey = _form64(recs)
    X0 = np.asarray(x0, np.float64) + 0.5 - cx
    Y0 = np.asarray(y0, np.float64) + 0.5 - cy
    X1, Y1 = X0 + (TILE - 1), Y0 + (TILE - 1)
    m00, m01, m11 = ax * ax + ex * ex, ax * ay + ex * ey, ay * ay + ey * ey

    def q(dx, dy):
        u, w = ax * dx + ay * dy, ex * dx + ey * dy
        return u * u + w * w
    with np.errstate(all="ignore"):
        out = np.full(cx.shape, np.inf)
        for xe in (X0, X1):                                   # edges x = const
            out = np.fmin(out, q(xe, np.clip(-m01 * xe / m11, Y0, Y1)))
        for ye in (Y0, Y1):                                   # edges y = const
            out = np.fmin(out, q(np.clip(-m01 * ye / m00, X0, X1), ye))
    inside = (X0 <= 0) & (X1 >= 0) & (Y0 <= 0) & (Y1 >= 0)
    return np.where(inside, 0.0, out)


# -- fp32: what the kernel computes ---------------------------------------------------------------------------------------------------
def quadrant_mask(rects, bx, by):
    """quadrant_mask of tile_blend.hip: bit (qx + 2 qy) for the tiles of bin (bx, by) inside the rect."""
    x0, y0, x1, y1 = rect_fields(rects)
    cx, cy = 2 * np.asarray(bx, np.int64), 2 * np.asarray(by, np.int64)
    mx = ((cx >= x0) & (cx <= x1)) * 1 | ((cx + 1 >= x0) & (cx + 1 <= x1)) * 2
    my = ((cy >= y0) & (cy <= y1)) * 1 | ((cy + 1 >= y0) & (cy + 1 <= y1)) * 2
    return ((mx & np.where(my & 1, 3, 0)) | ((mx & np.where(my & 2, 3, 0)) << 2)).astype(np.uint32)


def exact_quadrants32(recs, bx, by, variant="kernel"):
    """exact_quadrants of tile_blend.hip in np.float32, one rounding per operation (the kernel is compiled with contraction off),
    the reciprocal correctly rounded (v_rcp_f32 is within 1 ulp of it).  Returns the 4-bit mask of quadrants the test keeps, before it
    is and-ed with the rect's mask; a NaN anywhere keeps.  `variant` names a deliberately wrong version (the mutations the CPU tier
    must see fail) or "no_margin" (the 1.0001 margin removed)."""
    assert variant in VARIANTS
    f = np.float32
    cx, cy, ax, ay, ex, ey, _ = ref.rec_fields(recs)
    bx, by = np.broadcast_to(np.asarray(bx, np.int64), cx.shape), np.broadcast_to(np.asarray(by, np.int64), cx.shape)
    with np.errstate(all="ignore"):
        m00, m01, m11 = ax * ax + ex * ex, ax * ay + ex * ey, ay * ay + ey * ey
        r00, r11 = f(1.0) / m00, f(1.0) / m11
        if variant == "swap_rcp":
            r00, r11 = r11, r00
        limit = CUT32 if variant == "no_margin" else LIMIT32
        sign = f(1.0) if variant == "minimiser_sign" else f(-1.0)
        out = np.zeros(cx.shape, dtype=np.uint32)

        def form(dx, dy):
            if variant == "expanded":
                return (m00 * dx * dx + f(2.0) * m01 * dx * dy) + m11 * dy * dy
            u, w = ax * dx + ay * dy, ex * dx + ey * dy
            return u * u + w * w
        for r in range(2):
            Y0 = ((by * BIN + r * TILE).astype(f) + f(0.5)) - cy
            Y1 = Y0 + f(TILE - 1)
            yb = np.where(Y0 > 0, Y0, np.where(Y1 < 0, Y1, f(0.0))).astype(f)
            for c in range(2):
                X0 = ((bx * BIN + c * TILE).astype(f) + f(0.5)) - cx
                X1 = X0 + f(TILE - 1)
                xb = np.where(X0 > 0, X0, np.where(X1 < 0, X1, f(0.0))).astype(f)
                dy = np.fmin(np.fmax((sign * (m01 * xb)) * r11, Y0), Y1)
                q1 = np.where(xb != 0, form(xb, dy), HUGE32)
                dx = np.fmin(np.fmax((sign * (m01 * yb)) * r00, X0), X1)
                q2 = np.where(yb != 0, form(dx, yb), HUGE32)
                if variant == "one_edge":
                    qmin = q1
                elif variant == "max_not_min":
                    qmin = np.fmax(q1, q2)
                else:
                    qmin = np.fmin(q1, q2)
                qmin = np.where((xb != 0) | (yb != 0), qmin, f(0.0))
                out |= np.where(~(qmin > limit), np.uint32(1 << (c + 2 * r)), np.uint32(0))
    return out


def kernel_test32(recs, rects, bx, by, variant="kernel"):
    """The mask a composite kernel stages an entry with in bin (bx, by): quadrant_mask & exact_quadrants."""
    return quadrant_mask(rects, bx, by) & exact_quadrants32(recs, bx, by, variant)


# -- pairs ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Pairs:
    rec: np.ndarray          # int64 [P] index into the records
    tx: np.ndarray           # int64 [P] 16-px tile of the pair = quadrant (tx & 1) + 2 (ty & 1) of bin (tx >> 1, ty >> 1)
    ty: np.ndarray
    pmin64: np.ndarray       # float64 [P]
    boxmin64: np.ndarray     # float64 [P]
    keep32: np.ndarray       # bool [P]
    foot: np.ndarray         # int64 [P] pixels of the quadrant with power64 < CUT
    near: np.ndarray         # int64 [P] pixels within `band` of the cut
    band: float

    @property
    def must_keep(self):
        return self.pmin64 < CUT - self.band

    @property
    def must_drop(self):
        return self.boxmin64 > LIMIT + self.band

    @property
    def free(self):
        return ~self.must_keep & ~self.must_drop

    @property
    def bx(self):
        return self.tx >> 1

    @property
    def by(self):
        return self.ty >> 1

    @property
    def q(self):
        return (self.tx & 1) + 2 * (self.ty & 1)

    def kept_by(self, recs, rects, variant="kernel"):
        """bool [P]: whether kernel_test32 keeps each pair."""
        m = kernel_test32(recs[self.rec], rects[self.rec], self.bx, self.by, variant)
        return ((m >> self.q.astype(np.uint32)) & 1).astype(bool)

    def per_bin(self, sel, bins_x, bin_rows, bin_row_begin=0):
        """Pairs of `sel` counted per 32-px bin: int64 [bin_rows, bins_x]."""
        out = np.zeros((bin_rows, bins_x), dtype=np.int64)
        np.add.at(out, (self.by[sel] - bin_row_begin, self.bx[sel]), 1)
        return out


def live_rows(height, rows=None):
    """[y0, y1): the pixel rows of the frame, or of the strip of 16-px tile rows `rows`."""
    return (0, height) if rows is None else (rows[0] * TILE, min(rows[1] * TILE, height))


def analyse(recs, rects, vis, width, height, rows=None, band=BAND, only=None):
    """Every (visible record, live tile of its rect) pair of a frame, or of the strip `rows`, classed.  `only`: the record indexes to
    look at (default: every visible one)."""
    y0, y1 = live_rows(height, rows)
    idx = np.nonzero(vis)[0] if only is None else np.asarray(only, np.int64)[np.asarray(vis)[np.asarray(only, np.int64)]]
    rx0, ry0, rx1, ry1 = rect_fields(rects)
    rec, tx, ty = [], [], []
    for i in idx:
        xs, ys = np.arange(rx0[i], rx1[i] + 1), np.arange(ry0[i], ry1[i] + 1)
        ys = ys[(ys * TILE < y1) & (ys * TILE + TILE > y0)]                       # BinGeom::live
        xs = xs[xs * TILE < width]
        gy, gx = (a.ravel() for a in np.meshgrid(ys, xs, indexing="ij"))
        rec.append(np.full(gx.shape, i, dtype=np.int64)); tx.append(gx); ty.append(gy)
    rec, tx, ty = (np.concatenate(v) if v else np.zeros(0, np.int64) for v in (rec, tx, ty))
    P = rec.shape[0]
    pmin, keep32 = np.full(P, np.inf), np.zeros(P, dtype=bool)
    foot, near = np.zeros(P, np.int64), np.zeros(P, np.int64)
    key = ty * 65536 + tx
    order = np.argsort(key, kind="stable")
    cuts = np.nonzero(np.diff(key[order]))[0] + 1
    for grp in np.split(order, cuts):
        if grp.size == 0:
            continue
        qx, qy = int(tx[grp[0]]), int(ty[grp[0]])
        ys = np.arange(max(qy * TILE, y0), min(qy * TILE + TILE, y1))
        xs = np.arange(qx * TILE, min(qx * TILE + TILE, width))
        py, px = (a.ravel() for a in np.meshgrid(ys, xs, indexing="ij"))
        r = recs[rec[grp]]
        pw, pmin[grp] = pixel_power64(r, px, py)
        p32 = ref.power32(r, qx >> 1, qy >> 1, px, py)
        keep32[grp] = (p32 < CUT32).any(axis=1)
        foot[grp] = (pw < CUT).sum(axis=1)
        near[grp] = (np.abs(pw - CUT) <= band).sum(axis=1)
    box = box_min64(recs[rec], tx * TILE, ty * TILE) if P else np.zeros(0)
    return Pairs(rec, tx, ty, pmin, box, keep32, foot, near, band)


def measure_band(recs, rects, vis, width, height):
    """Worst |power32 - power64| over every (visible record, pixel with power64 < CUT + 1), every bin the record's rect reaches."""
    rx0, ry0, rx1, ry1 = rect_fields(rects)
    worst = 0.0
    for by in range((height + BIN - 1) // BIN):
        for bx in range((width + BIN - 1) // BIN):
            sel = vis & (rx0 <= 2 * bx + 1) & (rx1 >= 2 * bx) & (ry0 <= 2 * by + 1) & (ry1 >= 2 * by)
            if not sel.any():
                continue
            ys, xs = np.arange(by * BIN, min(height, by * BIN + BIN)), np.arange(bx * BIN, min(width, bx * BIN + BIN))
            py, px = (a.ravel() for a in np.meshgrid(ys, xs, indexing="ij"))
            worst = max(worst, ref.measure_alpha(recs[sel], bx, by, px, py)[0])
    return worst


# -- pixels: what a frame of a draw must show -----------------------------------------------------------------------------------------
def pixel_classes(recs, rects, splats, width, height, rows=None, band=BAND):
    """For a draw of the splats `splats` (visible ones): per pixel of the frame / strip (row 0 = the strip's first row)
    (sure bool [h, w] - some fragment whose tile the rect covers has power64 < CUT - band: the pixel is drawn;
     none bool [h, w] - every fragment has power64 > CUT + band or its rect does not cover the pixel's tile: the pixel stays clear;
     outside bool - some fragment with power64 < CUT - band lies outside its own rect: the vertex stage's bound would be wrong)."""
    y0, y1 = live_rows(height, rows)
    py, px = (a.ravel() for a in np.meshgrid(np.arange(y0, y1), np.arange(width), indexing="ij"))
    splats = np.asarray(splats, np.int64)
    pw = ref.power64(recs[splats], px, py)
    rx0, ry0, rx1, ry1 = (v[splats] for v in rect_fields(rects))
    tx, ty = px // TILE, py // TILE
    cover = (tx[None, :] >= rx0[:, None]) & (tx[None, :] <= rx1[:, None]) & (ty[None, :] >= ry0[:, None]) & (ty[None, :] <= ry1[:, None])
    shape = (y1 - y0, width)
    sure = (cover & (pw < CUT - band)).any(axis=0).reshape(shape)
    none = (~cover | (pw > CUT + band)).all(axis=0).reshape(shape)
    outside = (~cover & (pw < CUT - band)).any(axis=0).reshape(shape)
    return sure, none, outside
