"""Host model (numpy, fp64) of the surface pass, gs_mesh_surface: per pixel, the first entry of the pixel's near -> far list
after which the front-to-back transmittance has fallen to a threshold (include/gsplat_hip.h).

Its inputs are a draw's own intermediates - list ranges, entries, records, rects, slot-of-splat, the visibility mask
(gs_mesh_debug_read what = 2 / 8 / 0 / 1 / 9 / 3) - plus the centres and the camera.  It is NOT an equality oracle: the kernel's
alpha goes through v_exp_f32, which no host reproduces bit for bit.  It is a VALIDITY check with no pixel left out.  Per pixel it
keeps two transmittances:

    T_hi   skips every fragment whose fp64 power lies within ETA of the cut (power < 4 log2 e): the largest T the kernel may hold,
    T_lo   keeps them: the smallest.

An answer "entry k" is valid iff that entry can be a kept fragment (rect covers the pixel's tile, power < cut + ETA, depth test
passed), T_lo(k) <= tau + DELTA and T_hi(k - 1) > tau - DELTA; an answer "none" iff T_hi(end) > tau - DELTA.

DELTA does not grow with the walk: with a_j (1 + e_j), |e_j| <= eps, the absolute error of T_k is at most
sum_j T_{j-1} a_j eps = eps (1 - T_k) <= eps.  eps is the worst relative error of ONE fragment's alpha.

Measured (tests/test_surface_ref.py::test_the_tolerances_hold_on_the_test_scenes prints the figures and re-asserts them): the
kernel's staged fp32 expression (stage_entry + alpha_of of csrc/tile_blend.hip, restated below in np.float32 with every fma
rounded once) against fp64 over every (visible record, pixel) pair of the test scenes - helpers.small_scene(3000, 1, seed) at
150x90 for seeds 5 and 6 (the worst of all: seed 6) and the hand-made 64x64 scenes:
    worst |power_fp32 - power_fp64|                 2.523e-5   -> ETA       = 4 x = 1.01e-4
    worst relative error of alpha, fp32 vs fp64     1.748e-5   + 2^-22 = 2.4e-7 for the hardware exp2 = 1.772e-5
                                                               -> DELTA     = 4 x = 7.1e-5
    worst |depth_fp32 - depth_fp64|                 8.412e-8   -> DEPTH_TOL = 4 x = 3.4e-7
(the depth is the vertex stage's expression - v = MV c, q = P v, 0.5 q.z / q.w + 0.5, with MV = viewMatrix * transform formed
first under per-scene transforms - in np.float32, one rounding per operation, against the same expression in fp64 on the same
fp32 inputs; a window depth lies in [0, 1], so the tolerance is absolute).
"""
from dataclasses import dataclass

import numpy as np

NONE = 0xFFFFFFFF
TILE, BIN = 16, 32
CUT = float(np.float32(5.7707801636))          # GS_POWER_CUT as the kernel holds it
ETA = 1.01e-4
DELTA = 7.1e-5
DEPTH_TOL = 3.4e-7
EXP2_HW = 2.0 ** -22                           # v_exp_f32: 1 ulp


# -- the kernel's fp32 arithmetic, restated -------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fma in fp32: the product of two fp32 values is exact in fp64, so one fp64 add and one narrowing round once (double
    rounding only on exact ties of the fp64 sum: far below what is measured here)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def rec_fields(recs_u32):
    """uint32 [m, 8] records -> (cx, cy, ax, ay, bx, by float32 [m], alpha16 uint32 [m])."""
    r = np.ascontiguousarray(recs_u32, dtype=np.uint32).reshape(-1, 8)
    f = r[:, :6].copy().view(np.float32)
    return f[:, 0], f[:, 1], f[:, 2], f[:, 3], f[:, 4], f[:, 5], r[:, 7] >> 16


def power32(recs_u32, bin_x, bin_y, px, py):
    """The staged fp32 power of records [m] at pixels [p] of the 32-px bin (bin_x, bin_y): float32 [m, p]."""
    cx, cy, ax, ay, bx, by, _ = rec_fields(recs_u32)
    cxr = (cx - np.float32(bin_x * BIN)).astype(np.float32)
    cyr = (cy - np.float32(bin_y * BIN)).astype(np.float32)
    cu = -_fma32(ax, cxr, (ay * cyr).astype(np.float32))
    cw = -_fma32(bx, cxr, (by * cyr).astype(np.float32))
    fx = _f32(np.asarray(px) - bin_x * BIN) + np.float32(0.5)
    fy = _f32(np.asarray(py) - bin_y * BIN) + np.float32(0.5)
    ux = _fma32(ax[:, None], fx[None, :], cu[:, None])
    wx = _fma32(bx[:, None], fx[None, :], cw[:, None])
    u = _fma32(ay[:, None], fy[None, :], ux)
    w = _fma32(by[:, None], fy[None, :], wx)
    return _fma32(u, u, (w * w).astype(np.float32))


def power64(recs_u32, px, py):
    cx, cy, ax, ay, bx, by, _ = (np.asarray(v, np.float64) for v in rec_fields(recs_u32))
    dx = (np.asarray(px, np.float64) + 0.5)[None, :] - cx[:, None]
    dy = (np.asarray(py, np.float64) + 0.5)[None, :] - cy[:, None]
    u = ax[:, None] * dx + ay[:, None] * dy
    w = bx[:, None] * dx + by[:, None] * dy
    return u * u + w * w


def alpha64(recs_u32):
    return rec_fields(recs_u32)[6].astype(np.float64) / 65535.0


def measure_alpha(recs_u32, bin_x, bin_y, px, py):
    """(worst |power32 - power64|, worst relative error of the fp32 alpha incl. the hardware exp2's ulp) over records x pixels
    that come anywhere near the cut."""
    if len(recs_u32) == 0 or len(px) == 0:
        return 0.0, 0.0
    p32, p64 = power32(recs_u32, bin_x, bin_y, px, py), power64(recs_u32, px, py)
    near = p64 < CUT + 1.0
    if not near.any():
        return 0.0, 0.0
    a16 = rec_fields(recs_u32)[6]
    al32 = (a16.astype(np.float32) * np.float32(1.0 / 65535.0)).astype(np.float32)
    a32 = (np.exp2(-p32.astype(np.float64)).astype(np.float32) * al32[:, None]).astype(np.float32)
    a64 = np.exp2(-p64) * alpha64(recs_u32)[:, None]
    ok = near & (a64 > 0)
    rel = np.abs(a32.astype(np.float64) - a64)[ok] / a64[ok]
    return float(np.abs(p32.astype(np.float64) - p64)[near].max()), (float(rel.max()) if rel.size else 0.0) + EXP2_HW


# -- depth ----------------------------------------------------------------------------------------------------------------------
def model_view_of(view16, view_matrix16=None, transforms=None, scene_of_splat=None, n=0, dtype=np.float64):
    """Per-splat modelView [n, 16] (column-major): `view`, or view_matrix * transforms[scene] formed in `dtype` in the vertex
    stage's order."""
    if transforms is None:
        return np.broadcast_to(np.asarray(view16, np.float32).astype(dtype), (n, 16))
    A = np.asarray(view_matrix16, np.float32).astype(dtype)
    out = np.empty((len(transforms), 16), dtype=dtype)
    for s, t in enumerate(transforms):
        B = np.asarray(t, np.float64).astype(np.float32).astype(dtype)
        for col in range(4):
            for r in range(4):
                out[s, 4 * col + r] = ((A[r] * B[4 * col] + A[4 + r] * B[4 * col + 1]) + A[8 + r] * B[4 * col + 2]) + A[12 + r] * B[4 * col + 3]
    si = np.zeros(n, np.int64) if scene_of_splat is None else np.asarray(scene_of_splat, np.int64)
    return out[si]


def window_depth(centers, view16, proj16, dtype=np.float64, **dynamic):
    """0.5 * ndc.z + 0.5 of every centre, in `dtype` with one rounding per operation (np.float32 = the kernel's restatement)."""
    c = np.asarray(centers, np.float32).astype(dtype).reshape(-1, 3)
    MV = model_view_of(view16, n=c.shape[0], dtype=dtype, **dynamic)
    P = np.asarray(proj16, np.float32).astype(dtype)
    v = [((MV[:, r] * c[:, 0] + MV[:, 4 + r] * c[:, 1]) + MV[:, 8 + r] * c[:, 2]) + MV[:, 12 + r] for r in range(4)]
    q = [((P[r] * v[0] + P[4 + r] * v[1]) + P[8 + r] * v[2]) + P[12 + r] * v[3] for r in range(4)]
    with np.errstate(all="ignore"):
        return (q[2] / q[3]) * dtype(0.5) + dtype(0.5)


# -- the model ------------------------------------------------------------------------------------------------------------------
@dataclass
class Draw:
    """What a draw left behind (the caller's splat numbering throughout)."""
    width: int
    height: int
    list_shift: int                 # a list bin is (16 << list_shift) px
    lists_x: int
    list_row_begin: int
    ranges: np.ndarray              # uint32 [lists, 2]
    entries: np.ndarray             # uint32 [D] record slots
    slots: np.ndarray               # uint32 [n] slot of splat, NONE = not visible
    recs: np.ndarray                # uint32 [n, 8] by splat
    rects: np.ndarray               # uint32 [n, 2] by splat
    vis: np.ndarray                 # bool [n]
    z: np.ndarray                   # float64 [n] window depth of every centre
    dest_depth: np.ndarray = None   # float32 [H, W] or None
    unorm24: bool = False

    def splat_of_slot(self):
        m = np.full(int(self.slots[self.vis].max()) + 1 if self.vis.any() else 1, NONE, dtype=np.uint32)
        m[self.slots[self.vis]] = np.nonzero(self.vis)[0].astype(np.uint32)
        return m


def _depth_pass(draw, splats, px, py):
    """bool [m, p]: the blend's LEQUAL test of the splats' depth against the stored depth (fp64 model of either mode)."""
    if draw.dest_depth is None:
        return np.ones((len(splats), len(px)), dtype=bool)
    d = np.asarray(draw.dest_depth, np.float32)[py, px].astype(np.float64)
    z = draw.z[splats]
    if draw.unorm24:
        return np.floor(z * 16777215.0 + 0.5)[:, None] <= np.floor(d * 16777215.0 + 0.5)[None, :]
    return z[:, None] <= d[None, :]


def bin_transmittances(draw, bin_x, bin_y, px, py, smap=None, eta=ETA):
    """For the pixels (px, py) - all inside the 32-px bin (bin_x, bin_y) - the bin's candidate entries and both transmittances.
    Returns (splats uint32 [m] in list order, could_keep bool [m, p], T_lo, T_hi float64 [m, p])."""
    smap = draw.splat_of_slot() if smap is None else smap
    per = draw.list_shift - 1
    lid = ((bin_y >> per) - draw.list_row_begin) * draw.lists_x + (bin_x >> per)
    b, e = (int(v) for v in draw.ranges[lid])
    ent = draw.entries[b:e] if e > b else draw.entries[:0]
    splats = smap[ent]
    assert not (splats == NONE).any(), "a list names a record slot no visible splat owns"
    r = draw.rects[splats]
    x0, y0, x1, y1 = r[:, 0] & 0xFFFF, r[:, 0] >> 16, r[:, 1] & 0xFFFF, r[:, 1] >> 16
    touch = (x0 <= 2 * bin_x + 1) & (x1 >= 2 * bin_x) & (y0 <= 2 * bin_y + 1) & (y1 >= 2 * bin_y)
    splats = splats[touch]
    x0, y0, x1, y1 = x0[touch], y0[touch], x1[touch], y1[touch]
    tx, ty = np.asarray(px) // TILE, np.asarray(py) // TILE
    cover = (tx[None, :] >= x0[:, None]) & (tx[None, :] <= x1[:, None]) & (ty[None, :] >= y0[:, None]) & (ty[None, :] <= y1[:, None])
    cover &= _depth_pass(draw, splats, px, py)
    recs = draw.recs[splats]
    pw = power64(recs, px, py)
    a = np.exp2(-pw) * alpha64(recs)[:, None]
    could = cover & (pw < CUT + eta)
    sure = cover & (pw < CUT - eta)
    T_lo = np.cumprod(np.where(could, 1.0 - a, 1.0), axis=0)
    T_hi = np.cumprod(np.where(sure, 1.0 - a, 1.0), axis=0)
    return splats, could, T_lo, T_hi


def valid_answers(splats, could, T_lo, T_hi, tau, delta=DELTA):
    """Per pixel the set of valid answers: (ok bool [m, p] - entry k may be the answer; none_ok bool [p])."""
    m, p = T_lo.shape
    before = np.vstack([np.ones((1, p)), T_hi[:-1]]) if m else T_hi
    ok = could & (T_lo <= tau + delta) & (before > tau - delta)
    none_ok = (T_hi[-1] > tau - delta) if m else np.ones(p, dtype=bool)
    return ok, none_ok


def check_window(draw, x0, y0, ids, depth, tau, depth_tol=DEPTH_TOL, eta=ETA):
    """Every pixel of the window against the model.  Returns a list of complaints (empty = every pixel valid).  `eta`: the band
    around the cut in which a fragment may go either way, for scenes measured to need more than ETA (quadrant_ref.BAND)."""
    ids = np.asarray(ids)
    h, w = ids.shape
    bad = []
    smap = draw.splat_of_slot()
    for bin_y in range(y0 // BIN, (y0 + h - 1) // BIN + 1):
        for bin_x in range(x0 // BIN, (x0 + w - 1) // BIN + 1):
            ys = np.arange(max(y0, bin_y * BIN), min(y0 + h, bin_y * BIN + BIN))
            xs = np.arange(max(x0, bin_x * BIN), min(x0 + w, bin_x * BIN + BIN))
            py, px = (a.ravel() for a in np.meshgrid(ys, xs, indexing="ij"))
            splats, could, T_lo, T_hi = bin_transmittances(draw, bin_x, bin_y, px, py, smap, eta)
            ok, none_ok = valid_answers(splats, could, T_lo, T_hi, tau)
            got = ids[py - y0, px - x0]
            gz = np.asarray(depth)[py - y0, px - x0]
            where = {int(s): k for k, s in enumerate(splats)}
            for i in range(px.shape[0]):
                g = int(got[i])
                if g == NONE:
                    if not none_ok[i]:
                        bad.append(f"pixel ({px[i]}, {py[i]}): none, but T_hi(end) = {T_hi[-1, i]:.6f} <= tau - delta")
                    elif gz[i] != np.float32(1.0):
                        bad.append(f"pixel ({px[i]}, {py[i]}): none with depth {gz[i]!r}")
                    continue
                k = where.get(g)
                if k is None:
                    bad.append(f"pixel ({px[i]}, {py[i]}): splat {g} is not a candidate entry of the pixel's bin")
                elif not ok[k, i]:
                    prev = T_hi[k - 1, i] if k else 1.0
                    bad.append(f"pixel ({px[i]}, {py[i]}): splat {g} (entry {k}): T_lo = {T_lo[k, i]:.6f}, T_hi before = {prev:.6f}, "
                               f"could be kept = {bool(could[k, i])}, tau = {tau}")
                elif not abs(float(gz[i]) - draw.z[g]) <= depth_tol:
                    bad.append(f"pixel ({px[i]}, {py[i]}): depth {gz[i]!r} of splat {g}, fp64 {draw.z[g]!r}")
    return bad
