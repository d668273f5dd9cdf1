"""Host model of what decides visibility before and inside a strip's vertex stage (csrc/project.hip, csrc/mesh.hip).

Three pieces, all plain numpy:

  strip_planes     what a strip [r0, r1) of tile rows must hold, as a function of the FULL frame's planes.  Strip edges are
                   tile-aligned and the exact rect clip of k_project decides what passes, so there is no tolerance: the strip's
                   mask, rects and records are np.array_equal to this.
  vertical_extent  fp64 restatement of k_project's path from the covariance to ext_y (pinned to the raster oracle on the CPU).
  splat_reach,     fp64 restatements of the two hand-derived bounds that may drop a splat / a storage block before that path
  block_dead       runs: the per-splat strip pre-test and block_corner + block_misses_strip.  Their claim is
                   reach >= ext_y for every splat the full test keeps; test_strip_cull_ref.py checks it in fp64 and shows that
                   three named weakenings of the model break it on the case list.

The fp64 models are not bit-equal to the fp32 kernels and are never compared with device values of reach; the GPU tests use them
only to show that the cases exercise the bounds (splats kept although their centre lies outside the strip, blocks declared dead).
"""
from types import SimpleNamespace

import numpy as np

TILE = 16
RECT_EMPTY = (0xFFFF, 0)                 # what gs_mesh_debug_read(what = 1) reports for a splat that is not visible
WEAKENINGS = ("no_floor_term", "trace_bound", "no_row2")


# -- strips as a function of the full frame ---------------------------------------------------------------------------------------
def rect_fields(rects):
    r = np.asarray(rects, dtype=np.uint32)
    return r[:, 0] & 0xFFFF, r[:, 0] >> 16, r[:, 1] & 0xFFFF, r[:, 1] >> 16


def strip_planes(vis, rects, recs, r0, r1):
    """(mask bool [n], rects uint32 [n, 2], records uint32 [n, 8]) of the strip [r0, r1) from the full frame's: a splat is in the
    strip iff it is in the frame and its tile rows meet [r0, r1 - 1]; its rect keeps its columns and has its rows clamped to the
    strip; its record is the frame's.  Splats outside read (0xFFFF, 0) and a zero record, as the debug read reports them."""
    vis = np.asarray(vis, dtype=bool)
    x0, y0, x1, y1 = (f.astype(np.int64) for f in rect_fields(rects))
    mask = vis & (y0 <= r1 - 1) & (y1 >= r0) & (r1 > r0)
    ny0, ny1 = np.clip(y0, r0, None), np.clip(y1, None, r1 - 1)
    out_rects = np.empty((vis.shape[0], 2), dtype=np.uint32)
    out_rects[:, 0] = np.where(mask, x0 | (ny0 << 16), RECT_EMPTY[0]).astype(np.uint32)
    out_rects[:, 1] = np.where(mask, x1 | (ny1 << 16), RECT_EMPTY[1]).astype(np.uint32)
    out_recs = np.where(mask[:, None], np.asarray(recs, dtype=np.uint32), np.uint32(0))
    return mask, out_rects, out_recs


# -- uniforms -----------------------------------------------------------------------------------------------------------------------
def uniforms(cam, focal_adjustment=1.0, mesh_world=None, splat_scale=1.0, kernel2d=0.3, max_splat_px=1024.0, antialiased=False,
             point_cloud=False, dynamic=False):
    """What SplatMesh.set_camera hands the kernels, as fp64 copies of the fp32 values they read."""
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    fx, fy = cam.focal(focal_adjustment)
    return SimpleNamespace(view=f32(cam.model_view(mesh_world)).reshape(16), proj=f32(cam.projection).reshape(16),
                           view_matrix=f32(cam.view).reshape(16), focal_x=float(np.float32(fx)), focal_y=float(np.float32(fy)),
                           width=float(cam.width), height=float(cam.height), splat_scale=float(np.float32(splat_scale)),
                           inv_focal_adj=float(np.float32(1.0 / focal_adjustment)), kernel2d=float(np.float32(kernel2d)),
                           max_splat_px=float(np.float32(max_splat_px)), antialiased=bool(antialiased), point_cloud=bool(point_cloud),
                           orthographic=bool(getattr(cam, "is_orthographic", False)),
                           ortho_zoom=float(np.float32(getattr(cam, "zoom", 1.0))), dynamic=bool(dynamic),
                           tiles_y=(int(cam.height) + TILE - 1) // TILE)


def _mat(view):
    """column-major 16-vectors [..., 16] -> math matrices [m, 4, 4] (m = 1 or one per splat)."""
    return np.asarray(view, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)


def scene_views(view_matrix, transforms, dtype=np.float64):
    """viewMatrix * transform per scene, from the fp32 values the kernel reads and in its operation order: [scenes, 16]."""
    A = np.asarray(view_matrix, dtype=np.float64).astype(np.float32).astype(dtype).reshape(16)
    out = np.empty((len(transforms), 16), dtype=dtype)
    for s_, t in enumerate(transforms):
        B = np.asarray(t, dtype=np.float64).astype(np.float32).astype(dtype).reshape(16)
        for col in range(4):
            for r in range(4):
                out[s_, 4 * col + r] = A[r] * B[4 * col] + A[4 + r] * B[4 * col + 1] + A[8 + r] * B[4 * col + 2] + A[12 + r] * B[4 * col + 3]
    return out


def _view_space(M, centers):
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.einsum("mrc,nc->nr", M[:, :3, :3], c) + M[:, :3, 3] if M.shape[0] == 1 else \
            np.einsum("nrc,nc->nr", M[:, :3, :3], c) + M[:, :3, 3]


def _jacobian(u, v):
    n = v.shape[0]
    if u.orthographic:
        z = np.zeros(n)
        return z + u.ortho_zoom, z, z + u.ortho_zoom, z
    with np.errstate(all="ignore"):
        s = 1.0 / (v[:, 2] * v[:, 2])
        return u.focal_x / v[:, 2], -(u.focal_x * v[:, 0]) * s, u.focal_y / v[:, 2], -(u.focal_y * v[:, 1]) * s


def window_y(u, centers, view=None):
    """The window y of the centres (what the pre-test calls cyc), and whether the centre passes the vertex stage's frustum and
    depth rejects."""
    M = _mat(u.view if view is None else view)
    P = _mat(u.proj)[0]
    v = _view_space(M, centers)
    with np.errstate(all="ignore"):
        q = np.concatenate([v, np.ones((v.shape[0], 1))], axis=1) @ P.T
        clip = 1.2 * q[:, 3]
        ok = ~((q[:, 2] < -clip) | (q[:, 0] < -clip) | (q[:, 0] > clip) | (q[:, 1] < -clip) | (q[:, 1] > clip))
        ndc = q[:, :3] / q[:, 3:4]
        ok &= (ndc[:, 2] >= -1.0) & (ndc[:, 2] <= 1.0)
        return (ndc[:, 1] * 0.5 + 0.5) * u.height, ok


# -- covariance -> ext_y ----------------------------------------------------------------------------------------------------------
def vertical_extent(u, centers, cov, view=None, dtype=np.float64):
    """k_project from the 3D covariance to the quad's vertical half extent: J, T = W J, cov2D = T' V T, + kernel2d, the
    eigenvalues with the discriminant floored at 0.1 (or 0.2 twice in point-cloud mode), the basis, the max_splat_px clamp and
    splat_scale * inv_focal_adj - in fp64, written in the kernel's operation order.  dtype = np.float32 evaluates the same
    statements in the kernel's own precision: the basis of a needle that lies along a screen axis comes from the cancelling
    difference l1 - a, so only an evaluation in the same precision can be pinned to the fp32 oracle component by component.
    `view`: one modelView per splat (per-scene transforms) instead of u.view.  Returns ok (the splat survives this path: l2 > 0 and a
    finite basis), the basis in pixels (b1x, b1y, b2x, b2y), raw = sqrt(b1y^2 + b2y^2) and ext_y = raw * 1.00001 + 1e-3, the
    padded value the rect clip uses."""
    f = dtype
    M = _mat(u.view if view is None else view).astype(f)
    c = np.asarray(centers).reshape(-1, 3).astype(f)
    V00, V01, V02, V11, V12, V22 = (np.asarray(cov).reshape(-1, 6)[:, k].astype(f) for k in range(6))
    fx, fy, kern, cap = f(u.focal_x), f(u.focal_y), f(u.kernel2d), f(u.max_splat_px)
    with np.errstate(all="ignore"):
        v = [M[:, r, 0] * c[:, 0] + M[:, r, 1] * c[:, 1] + M[:, r, 2] * c[:, 2] + M[:, r, 3] for r in range(3)]
        if u.orthographic:
            j00 = j11 = np.full(c.shape[0], u.ortho_zoom, dtype=f)
            j20 = j21 = np.zeros(c.shape[0], dtype=f)
        else:
            s = f(1.0) / (v[2] * v[2])
            j00, j20 = fx / v[2], -(fx * v[0]) * s
            j11, j21 = fy / v[2], -(fy * v[1]) * s
        T0 = [M[:, 0, r] * j00 + M[:, 2, r] * j20 for r in range(3)]
        T1 = [M[:, 1, r] * j11 + M[:, 2, r] * j21 for r in range(3)]
        VT = lambda T: [V00 * T[0] + V01 * T[1] + V02 * T[2], V01 * T[0] + V11 * T[1] + V12 * T[2], V02 * T[0] + V12 * T[1] + V22 * T[2]]
        VT0, VT1 = VT(T0), VT(T1)
        a = T0[0] * VT0[0] + T0[1] * VT0[1] + T0[2] * VT0[2] + kern
        b = T0[0] * VT1[0] + T0[1] * VT1[1] + T0[2] * VT1[2]
        d = T1[0] * VT1[0] + T1[1] * VT1[1] + T1[2] * VT1[2] + kern
        D = a * d - b * b
        half_tr = f(0.5) * (a + d)
        disc = half_tr * half_tr - D
        term2 = np.sqrt(np.where(disc > f(0.1), disc, f(0.1)))
        l1, l2 = half_tr + term2, half_tr - term2
        if u.point_cloud:
            l1, l2 = np.full_like(l1, f(0.2)), np.full_like(l2, f(0.2))
        ex, ey = b, l1 - a
        elen = np.sqrt(ex * ex + ey * ey)
        e1x, e1y = ex / elen, ey / elen
        ok = (l2 > 0) & np.isfinite(e1x) & np.isfinite(e1y)
        sqrt8 = np.sqrt(f(8.0))
        h1, h2 = np.minimum(sqrt8 * np.sqrt(l1), cap), np.minimum(sqrt8 * np.sqrt(l2), cap)
        k = f(u.splat_scale) * f(u.inv_focal_adj)
        b1x, b1y, b2x, b2y = e1x * k * h1, e1y * k * h1, e1y * k * h2, -e1x * k * h2
        raw = np.sqrt(b1y * b1y + b2y * b2y)
        return SimpleNamespace(ok=ok, b1x=b1x, b1y=b1y, b2x=b2x, b2y=b2y, raw=raw, ext_y=raw * f(1.00001) + f(1e-3))


# -- the bounds ---------------------------------------------------------------------------------------------------------------------
def cov_bound(cov, weaken=None):
    """cov_spectral_bound of mesh.hip: the largest absolute row sum (Gershgorin; NaN in, NaN out), times 1.00001.
    weaken = "trace_bound": trace / 3, the mean eigenvalue - not a bound."""
    c = np.asarray(cov, dtype=np.float64).reshape(-1, 6)
    if weaken == "trace_bound":
        return (c[:, 0] + c[:, 3] + c[:, 5]) / 3.0
    a = np.abs(c)
    with np.errstate(all="ignore"):
        rows = np.stack([a[:, 0] + a[:, 1] + a[:, 2], a[:, 1] + a[:, 3] + a[:, 4], a[:, 2] + a[:, 4] + a[:, 5]], axis=1)
        return rows.max(axis=1) * 1.00001                     # (max propagates NaN)


def _row_norms(u):
    M = _mat(u.view)[0]
    return np.sqrt((M[:3, :3] ** 2).sum(axis=1)) * (1.0 + 1e-6)


def _cap(u):
    return u.max_splat_px * abs(u.splat_scale * u.inv_focal_adj) * 1.001 + 2.0


def splat_reach(u, centers, bound, weaken=None):
    """The per-splat strip pre-test of k_project: how far from its centre's window y a splat may reach, from the centre and the
    4-byte covariance bound alone.  Per-scene transforms (u.dynamic) fall back to the screen-size cap, and so does a NaN."""
    n = np.asarray(centers).reshape(-1, 3).shape[0]
    cap = np.full(n, _cap(u))
    if u.dynamic:
        return cap
    v = _view_space(_mat(u.view), centers)
    j00, j20, j11, j21 = _jacobian(u, v)
    rn = _row_norms(u)
    row2 = 0.0 if weaken == "no_row2" else rn[2]
    ks = abs(u.splat_scale * u.inv_focal_adj)
    with np.errstate(all="ignore"):
        t = np.maximum(np.abs(j00) * rn[0] + np.abs(j20) * row2, np.abs(j11) * rn[1] + np.abs(j21) * row2) * 1.0001
        l = np.asarray(bound, dtype=np.float64) * t * t + u.kernel2d + (0.0 if weaken == "no_floor_term" else 0.3163)
        if u.point_cloud:
            l = np.fmax(l, 0.2)
        tight = ks * np.sqrt(8.0 * l) * 1.001 + 2.0
        return np.where(tight < cap, tight, cap)


def pretest_keeps(u, centers, bound, r0, r1, weaken=None, view=None):
    """True where the pre-test lets a centre that passed the frustum go on to the exact test of the strip [r0, r1)."""
    cyc, ok = window_y(u, centers, view)
    reach = splat_reach(u, centers, bound, weaken)
    with np.errstate(all="ignore"):
        return ok & ~((cyc + reach < r0 * TILE) | (cyc - reach > r1 * TILE))


def block_boxes(centers, bound, position, blocks):
    """k_block_boxes: per storage block (position // 256) the min / max of its members' centres, NaN left out per coordinate, the
    largest member bound (NaN if any member's is NaN) and an unused eighth float (reported as 0 here; the device leaves it 0)."""
    c = np.asarray(centers, dtype=np.float32).reshape(-1, 3)
    b = np.asarray(bound, dtype=np.float32)
    blk = np.asarray(position, dtype=np.int64) // 256
    out = np.zeros((blocks, 8), dtype=np.float32)
    out[:, 0:3], out[:, 3:6] = np.inf, -np.inf
    for k in range(3):
        np.fmin.at(out[:, k], blk, c[:, k])
        np.fmax.at(out[:, 3 + k], blk, c[:, k])
    np.fmax.at(out[:, 6], blk, b)
    has_nan = np.zeros(blocks, dtype=bool)
    np.logical_or.at(has_nan, blk, np.isnan(b))
    out[has_nan, 6] = np.nan
    return out


def block_dead(u, boxes, r0, r1):
    """block_corner + block_misses_strip over block_box rows [blocks, 8]: (dead by the frustum, dead by the strip [r0, r1) alone).
    The strip half stands down for an orthographic camera, for the full frame and unless all eight corners are in front."""
    bb = np.asarray(boxes, dtype=np.float64).reshape(-1, 8)
    nb = bb.shape[0]
    sel = np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)])
    corners = np.where(sel[None, :, :] == 1, bb[:, None, 3:6], bb[:, None, 0:3])                # [blocks, 8, 3]
    M, P = _mat(u.view)[0], _mat(u.proj)[0]
    with np.errstate(all="ignore"):
        v = corners @ M[:3, :3].T + M[:3, 3]
        q = np.concatenate([v, np.ones((nb, 8, 1))], axis=2) @ P.T
        clip = 1.2 * q[..., 3]
        tol = 1e-4 * (np.abs(q[..., 0]) + np.abs(q[..., 1]) + np.abs(q[..., 2]) + np.abs(clip) + 1.0)
        rej = np.stack([q[..., 0] - clip > tol, -q[..., 0] - clip > tol, q[..., 1] - clip > tol, -q[..., 1] - clip > tol,
                        -q[..., 2] - clip > tol, -q[..., 3] > tol], axis=2)
        dead_frustum = rej.all(axis=1).any(axis=1)
        front = ((q[..., 3] > 1e-6) & (v[..., 2] < -1e-6)).all(axis=1)
        ypx = (q[..., 1] / q[..., 3] * 0.5 + 0.5) * u.height
        ymin, ymax = np.fmin.reduce(ypx, axis=1), np.fmax.reduce(ypx, axis=1)
        zmin = np.fmin.reduce(-v[..., 2], axis=1)
        axmax, aymax = np.fmax.reduce(np.abs(v[..., 0]), axis=1), np.fmax.reduce(np.abs(v[..., 1]), axis=1)
        ks = abs(u.splat_scale * u.inv_focal_adj)
        rn = _row_norms(u)
        iz = 1.0 / zmin
        t0 = abs(u.focal_x) * iz * rn[0] + abs(u.focal_x) * axmax * iz * iz * rn[2]
        t1 = abs(u.focal_y) * iz * rn[1] + abs(u.focal_y) * aymax * iz * iz * rn[2]
        t = np.maximum(t0, t1) * 1.001
        l = bb[:, 6] * t * t + u.kernel2d + 0.3163
        if u.point_cloud:
            l = np.fmax(l, 0.2)
        tight = ks * np.sqrt(8.0 * l) * 1.002 + 2.0
        reach = np.where(tight < _cap(u), tight, _cap(u))
        slack = 0.05 + 1e-5 * u.height
        miss = (ymax + reach + slack < r0 * TILE) | (ymin - reach - slack > r1 * TILE)
    is_strip = r0 > 0 or r1 < u.tiles_y
    stands = is_strip and not u.orthographic and not u.dynamic
    return dead_frustum, (~dead_frustum & front & miss) if stands else np.zeros(nb, dtype=bool)
