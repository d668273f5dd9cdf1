"""Host model of SplatRenderMode.TwoD (the reference's SplatMaterial2D, useRefImplementation = false) in np.float32, every product
and sum rounded on its own in the shader's stated order - what csrc/project_2d.hip and csrc/tile_blend_2d.hip restate on the device.

  vertex(case)             SplatMaterial.buildVertexShaderBase (SH 0 / 1 / 2, fp16 or 8-bit) + SplatMaterial2D.buildVertexShaderProjection
                           (/root/reference/src/splatmesh/SplatMaterial2D.js:94-236) -> the engine's 80-byte records
  fragments(...)           SplatMaterial2D.buildFragmentShader (:302-343) per (splat, pixel), plus which pixels are AMBIGUOUS
  composite_fp32 / _rop8   front to back in fp32, rounded once | back to front, rounded to 8 bits after every splat

A pixel is ambiguous where some (splat, pixel) decision - inside the quad, p.z == 0, rho3d <= rho2d, depth < 0.2, alpha < 1/255, the
depth test - flips under a relative perturbation of 1e-4 of the compared quantity, or a quad edge passes within 1/256 px of the
pixel's centre (a rasteriser's subpixel grid).

MUTATIONS name single-line changes of the chain; tests/test_surfel_ref.py holds the cases to telling each of them apart.
"""
import numpy as np

f32 = np.float32
MUTATIONS = ("rho2d_dropped", "min_is_rho3d", "near_removed", "cap_removed", "factor3_sqrt8", "ifa_omitted", "minpix_never",
             "minpix_always", "missing_w_negated", "t_transposed", "ndc2pix_minus1_omitted")
REL = f32(1e-4)


def make_case(centers, scales, rotations, rgba, cam, inv_focal_adj=1.0, scene_idx=None, transforms=None, opacity=None, visible=None,
              fade=None, sh=None, sh_degree=0, sh8_range=None):
    """A scene and its uniforms.  scales / rotations as SplatBuffer.fillSplatScaleRotationArray returns them (rotation x, y, z, w,
    normalised, w >= 0); scale z is overridden to 1 as SplatMesh.fillSplatDataArrays does in 2D mode.  sh: what the mesh stores,
    float16 [n, 9 | 24] coefficient-major RGB triples, or uint8 with sh8_range = (min, max) of the 8-bit compression."""
    n = len(centers)
    sc = np.array(scales, f32).reshape(n, 3)
    sc[:, 2] = 1.0
    tuples = np.concatenate([sc, np.asarray(rotations, f32).reshape(n, 4)[:, :3]], axis=1)
    return dict(centers=np.asarray(centers, f32).reshape(n, 3), scales=np.asarray(scales, f32).reshape(n, 3),
                rotations=np.asarray(rotations, f32).reshape(n, 4), tuples=tuples, rgba=np.asarray(rgba, np.uint8).reshape(n, 4),
                camera=cam, width=int(cam.width), height=int(cam.height), view=np.asarray(cam.model_view(), np.float64).astype(f32).reshape(16),
                proj=np.asarray(cam.projection, np.float64).astype(f32).reshape(16),
                view_matrix=np.asarray(cam.view, np.float64).astype(f32).reshape(16), inv_focal_adj=f32(inv_focal_adj),
                scene_idx=None if scene_idx is None else np.asarray(scene_idx, np.uint32),
                transforms=None if transforms is None else [np.asarray(t, np.float64).astype(f32).reshape(16) for t in transforms],
                opacity=opacity, visible=visible, fade=fade, sh=sh, sh_degree=int(sh_degree), sh8_range=sh8_range,
                cam_pos=np.asarray(cam.position, f32))


def _unorm16(v):
    return (np.clip(v, f32(0), f32(1)) * f32(65535.0) + f32(0.5)).astype(np.uint32)


def vertex(case, mut=()):
    """-> dict of per-splat arrays: visible, branch (1 = the AABB square, 0 = the parallelogram), tu / tv / tw [n,3], qc [n,2],
    c [n,2], inv [n,4], c0, c1 (unorm16 words), rect [n,4] (tile x0, y0, x1, y1), zwin."""
    with np.errstate(all="ignore"):
        return _vertex(case, mut)


def _vertex(case, mut):
    c = case["centers"]
    n = c.shape[0]
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    W, H = f32(case["width"]), f32(case["height"])
    P = case["proj"]
    scene = case["scene_idx"] if case["scene_idx"] is not None else np.zeros(n, np.uint32)
    ok = np.ones(n, bool)
    if case["opacity"] is not None:                            # enableOptionalEffects (SplatMaterial.js:129-137): the reject only
        op, vi = np.asarray(case["opacity"], f32), np.asarray(case["visible"], np.uint32)
        ok &= ~((op[scene] <= f32(0.01)) | (vi[scene] == 0))
    if case["transforms"] is not None:                         # dynamicMode (:140-144): viewMatrix * transform, per scene
        A = case["view_matrix"]
        per = []
        for B in case["transforms"]:
            m = np.empty(16, f32)
            for col in range(4):
                for r in range(4):
                    m[4 * col + r] = A[r] * B[4 * col] + A[4 + r] * B[4 * col + 1] + A[8 + r] * B[4 * col + 2] + A[12 + r] * B[4 * col + 3]
            per.append(m)
        MV = np.stack(per)[scene].T                            # [16, n]
    else:
        MV = np.repeat(case["view"][:, None], n, axis=1)
    v = [MV[r] * x + MV[4 + r] * y + MV[8 + r] * z + MV[12 + r] for r in range(4)]
    q = [P[r] * v[0] + P[4 + r] * v[1] + P[8 + r] * v[2] + P[12 + r] * v[3] for r in range(4)]
    clip = f32(1.2) * q[3]
    ok &= ~((q[2] < -clip) | (q[0] < -clip) | (q[0] > clip) | (q[1] < -clip) | (q[1] > clip))
    ndcx, ndcy, ndcz = q[0] / q[3], q[1] / q[3], q[2] / q[3]
    ok &= (ndcz >= f32(-1)) & (ndcz <= f32(1))
    zwin = ndcz * f32(0.5) + f32(0.5)
    rgba = case["rgba"].astype(f32) * (f32(1.0) / f32(255.0))
    alpha = rgba[:, 3].copy()
    col = [rgba[:, 0], rgba[:, 1], rgba[:, 2]]
    if case["sh_degree"] >= 1:                                 # SplatMaterial.js:179-337, in csrc/project_common.hpp's order
        if case["transforms"] is not None:                     # dynamicMode: the camera in the scene's own frame (fp64 on the host)
            inv = [np.linalg.inv(np.asarray(t, np.float64).reshape(4, 4).T) @ np.array([*case["cam_pos"].astype(np.float64), 1.0])
                   for t in case["transforms"]]
            cp = np.stack(inv)[:, :3].astype(f32)[scene].T
        else:
            cp = case["cam_pos"]
        d0, d1, d2 = x - cp[0], y - cp[1], z - cp[2]
        inv = f32(1.0) / np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
        dx_, dy_, dz_ = d0 * inv, d1 * inv, d2 * inv
        if case["sh8_range"] is not None:                      # texel = byte / 255, sh = texel * range + min
            mn = f32(case["sh8_range"][0])
            rng_ = f32(case["sh8_range"][1]) - mn
            sh = (case["sh"].astype(f32) / f32(255.0)) * rng_ + mn
        else:
            sh = np.asarray(case["sh"]).view(np.float16).astype(f32) if np.asarray(case["sh"]).dtype == np.uint16 else np.asarray(case["sh"], np.float16).astype(f32)
        C1 = f32(0.4886025119029199)
        for ch in range(3):
            col[ch] = col[ch] + C1 * (-sh[:, 0 + ch] * dy_ + sh[:, 3 + ch] * dz_ - sh[:, 6 + ch] * dx_)
        if case["sh_degree"] >= 2:
            xx, yy, zz, xy, yz, xz = dx_ * dx_, dy_ * dy_, dz_ * dz_, dx_ * dy_, dy_ * dz_, dx_ * dz_
            K0, K1, K2, K3, K4 = f32(1.0925484), f32(-1.0925484), f32(0.3153916), f32(-1.0925484), f32(0.5462742)
            for ch in range(3):
                col[ch] = col[ch] + ((K0 * xy) * sh[:, 9 + ch] + (K1 * yz) * sh[:, 12 + ch] + (K2 * (f32(2.0) * zz - xx - yy)) * sh[:, 15 + ch] +
                                     (K3 * xz) * sh[:, 18 + ch] + (K4 * (xx - yy)) * sh[:, 21 + ch])
        col = [np.clip(c_, f32(0), f32(1)) for c_ in col]
    t = case["tuples"]
    s0, s1, qx, qy, qz = t[:, 0], t[:, 1], t[:, 3], t[:, 4], t[:, 5]
    qw = np.sqrt(f32(1.0) - qx * qx - qy * qy - qz * qz)
    if "missing_w_negated" in mut:
        qw = -qw
    two, one = f32(2.0), f32(1.0)
    R0 = [one - two * (qy * qy + qz * qz), two * (qx * qy + qw * qz), two * (qx * qz - qw * qy)]
    R1 = [two * (qx * qy - qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz + qw * qx)]
    L0 = [R0[k] * s0 for k in range(3)]
    L1 = [R1[k] * s1 for k in range(3)]
    M = [None] * 16
    for k in range(4):
        for r in range(4):
            M[4 * k + r] = P[r] * MV[4 * k] + P[4 + r] * MV[4 * k + 1] + P[8 + r] * MV[4 * k + 2] + P[12 + r] * MV[4 * k + 3]
    X = [[L0[0] * M[cc] + L0[1] * M[4 + cc] + L0[2] * M[8 + cc], L1[0] * M[cc] + L1[1] * M[4 + cc] + L1[2] * M[8 + cc],
          x * M[cc] + y * M[4 + cc] + z * M[8 + cc] + M[12 + cc]] for cc in range(4)]
    hw, hh = W / two, H / two
    hwm, hhm = ((W - one) / two, (H - one) / two) if "ndc2pix_minus1_omitted" not in mut else (hw, hh)
    Tu = [X[0][r] * hw + X[3][r] * hwm for r in range(3)]
    Tv = [X[1][r] * hh + X[3][r] * hhm for r in range(3)]
    Tw = [X[3][r] for r in range(3)]
    if "t_transposed" in mut:
        Tu, Tv, Tw = [Tu[0], Tv[0], Tw[0]], [Tu[1], Tv[1], Tw[1]], [Tu[2], Tv[2], Tw[2]]
    p1 = [X[cc][0] + X[cc][2] for cc in range(4)]
    p2 = [X[cc][1] + X[cc][2] for cc in range(4)]
    pc = [X[cc][2] for cc in range(4)]
    p1x, p1y, p2x, p2y = p1[0] / p1[3], p1[1] / p1[3], p2[0] / p2[3], p2[1] / p2[3]
    pcx, pcy = pc[0] / pc[3], pc[1] / pc[3]
    b1x, b1y, b2x, b2y = p1x - pcx, p1y - pcy, p2x - pcx, p2y - pcy
    half = f32(0.5)
    b1sx, b1sy, b2sx, b2sy = b1x * half * W, b1y * half * H, b2x * half * W, b2y * half * H
    len1, len2 = np.sqrt(b1sx * b1sx + b1sy * b1sy), np.sqrt(b2sx * b2sx + b2sy * b2sy)
    small = (len1 < one) | (len2 < one)
    if "minpix_never" in mut:
        small = np.zeros(n, bool)
    if "minpix_always" in mut:
        small = np.ones(n, bool)
    three = f32(3.0) if "factor3_sqrt8" not in mut else np.sqrt(f32(8.0))
    ifa = case["inv_focal_adj"] if "ifa_omitted" not in mut else one
    # the AABB branch (:160-188)
    distance = Tw[0] * Tw[0] * one + Tw[1] * Tw[1] * one + Tw[2] * Tw[2] * -one
    inv = one / distance
    f0, f1, f2 = inv * one, inv * one, inv * -one
    pix = Tu[0] * Tw[0] * f0 + Tu[1] * Tw[1] * f1 + Tu[2] * Tw[2] * f2
    piy = Tv[0] * Tw[0] * f0 + Tv[1] * Tw[1] * f1 + Tv[2] * Tw[2] * f2
    tx = Tu[0] * Tu[0] * f0 + Tu[1] * Tu[1] * f1 + Tu[2] * Tu[2] * f2
    ty = Tv[0] * Tv[0] * f0 + Tv[1] * Tv[1] * f1 + Tv[2] * Tv[2] * f2
    ex = np.sqrt(np.maximum(f32(0.0001), pix * pix - tx))
    ey = np.sqrt(np.maximum(f32(0.0001), piy * piy - ty))
    radius = np.maximum(ex, ey)
    bvx, bvy = one / W, one / H
    ok &= ~(small & (np.abs(distance) < f32(0.00001)))
    zero = np.zeros(n, f32)
    B1x = np.where(small, radius * three * bvx * two * half * W, b1x * three * ifa * half * W)
    B1y = np.where(small, zero, b1y * three * ifa * half * H)
    B2x = np.where(small, zero, b2x * three * ifa * half * W)
    B2y = np.where(small, radius * three * bvy * two * half * H, b2y * three * ifa * half * H)
    qcx, qcy = np.where(small, pix, pcx), np.where(small, piy, pcy)
    if case["fade"] is not None:                               # SplatMaterial.js:347-363
        sc_, start = np.asarray(case["fade"][0], f32), f32(case["fade"][1])
        fx_, fy_, fz_ = x - sc_[0], y - sc_[1], z - sc_[2]
        dist = np.sqrt(fx_ * fx_ + fy_ * fy_ + fz_ * fz_)
        f = np.where(dist < start, f32(0), f32(1))
        tt = np.clip((dist - start) / f32(0.75), f32(0), f32(1))
        f = (one - f) + (one - tt) * f
        alpha = alpha * (one * f)
    cx, cy = (ndcx * half + half) * W, (ndcy * half + half) * H
    ext_x = (np.abs(B1x) + np.abs(B2x)) * f32(1.00001) + f32(1e-3)
    ext_y = (np.abs(B1y) + np.abs(B2y)) * f32(1.00001) + f32(1e-3)
    fx0, fx1 = np.ceil(cx - ext_x - half), np.floor(cx + ext_x - half)
    fy0, fy1 = np.ceil(cy - ext_y - half), np.floor(cy + ext_y - half)
    fx0, fx1 = np.maximum(fx0, f32(0)), np.minimum(fx1, W - one)
    fy0, fy1 = np.maximum(fy0, f32(0)), np.minimum(fy1, H - one)
    det = B1x * B2y - B2x * B1y
    vis = ok & (fx0 <= fx1) & (fy0 <= fy1) & (det == det)
    px = np.stack([np.where(vis, a, 0) for a in (fx0, fy0, fx1, fy1)], axis=1).astype(np.int64)
    out = dict(visible=vis, branch=small.astype(np.uint8), tu=np.stack(Tu, 1), tv=np.stack(Tv, 1), tw=np.stack(Tw, 1),
               qc=np.stack([qcx, qcy], 1), c=np.stack([cx, cy], 1),
               inv=np.stack([B2y / det, -B2x / det, -B1y / det, B1x / det], 1), zwin=zwin, pixel_rect=px, rect=px // 16,
               c0=_unorm16(col[0]) | (_unorm16(col[1]) << 16), c1=_unorm16(col[2]) | (_unorm16(alpha) << 16),
               len=np.stack([len1, len2], 1), distance=distance, basis=np.stack([B1x, B1y, B2x, B2y], 1), ndcz=ndcz)
    return out


def gl_distances(v, cap, width, height):
    """The model's vertex outputs against a transform-feedback capture of the reference's shader (tests/golden/surfel_gl_ref*.npz:
    `cap` float32 [m, 24] = gl_Position.xy of the 4 corners, gl_Position.z, vColor, vT column by column, vQuadCenter, for the
    splats `written`): the largest distance per field class over the splats the model draws - quad centre and basis vectors in
    pixels (the viewport transform of the corners), rows of vT relative to the row's norm, vQuadCenter in pixels (its NDC value
    scaled by half the viewport in the parallelogram branch), colour in unorm16 units."""
    with np.errstate(all="ignore"):                            # (rows of splats nobody draws may be zero or NaN: the callers mask them)
        return _gl_distances(v, cap, width, height)


def _gl_distances(v, cap, width, height):
    W, H = np.float64(width), np.float64(height)
    cap = cap.astype(np.float64)
    cx = (cap[:, 0:8:2] * 0.5 + 0.5) * W                       # corners (-1,-1), (-1,1), (1,1), (1,-1)
    cy = (cap[:, 1:8:2] * 0.5 + 0.5) * H
    centre = np.stack([cx.mean(axis=1), cy.mean(axis=1)], 1)
    basis = np.stack([(cx[:, 3] - cx[:, 0]) / 2, (cy[:, 3] - cy[:, 0]) / 2, (cx[:, 1] - cx[:, 0]) / 2, (cy[:, 1] - cy[:, 0]) / 2], 1)
    out = {"centre_px": np.abs(centre - v["c"]).max(axis=1), "basis_px": np.abs(basis - v["basis"]).max(axis=1)}
    rows = []
    for k, key in enumerate(("tu", "tv", "tw")):
        got, want = cap[:, 13 + 3 * k:16 + 3 * k], v[key].astype(np.float64)
        rows.append(np.abs(got - want).max(axis=1) / np.linalg.norm(want, axis=1))
    out["t_rows_rel"] = np.max(rows, axis=0)
    scale = np.where(v["branch"][:, None] == 1, 1.0, np.array([W / 2, H / 2]))
    out["quad_center_px"] = (np.abs(cap[:, 22:24] - v["qc"]) * scale).max(axis=1)
    k16 = 1.0 / 65535.0
    want = np.stack([v["c0"] & 0xFFFF, v["c0"] >> 16, v["c1"] & 0xFFFF, v["c1"] >> 16], 1).astype(np.float64) * k16
    out["colour_unorm16"] = np.abs(np.clip(cap[:, 9:13], 0, 1) - want).max(axis=1) * 65535.0
    out["ndcz"] = np.abs(cap[:, 8] - v["ndcz"])
    return out


def records(v):
    """The vertex stage's outputs as the engine's 20-word records (float32 view of words 0..16)."""
    n = v["visible"].shape[0]
    r = np.zeros((n, 20), np.uint32)
    fl = np.concatenate([v["tu"], v["tv"], v["tw"], v["qc"], v["c"], v["inv"]], axis=1).astype(f32)
    r[:, :17] = fl.view(np.uint32)
    r[:, 17], r[:, 18] = v["c0"], v["c1"]
    r[~v["visible"]] = 0
    return r


def fragments(v, i, xs, ys, mut=(), dest_depth=None, depth_unorm24=False):
    """Splat i of vertex() output v on the pixels (xs, ys) (integer arrays): -> (alpha float32, 0 where no fragment is blended;
    ambiguous bool)."""
    with np.errstate(all="ignore"):
        fx, fy = xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)
        tu, tv, tw, qc, c, iv = v["tu"][i], v["tv"][i], v["tw"][i], v["qc"][i], v["c"][i], v["inv"][i]
        opa = f32((int(v["c1"][i]) >> 16)) * (f32(1.0) / f32(65535.0))
        dx, dy = fx - c[0], fy - c[1]
        u, w = iv[0] * dx + iv[1] * dy, iv[2] * dx + iv[3] * dy
        inside = (np.abs(u) <= f32(1)) & (np.abs(w) <= f32(1))
        nu, nw = np.hypot(iv[0], iv[1]), np.hypot(iv[2], iv[3])          # 1 / (distance between the quad's opposite edges / 2)
        du, dw = np.abs(np.abs(u) - f32(1)), np.abs(np.abs(w) - f32(1))
        near_edge = ((du <= REL) | (du / nu <= f32(1.0 / 256.0))) & (np.abs(w) <= f32(1) + REL + f32(1.0 / 256.0) * nw)
        near_edge |= ((dw <= REL) | (dw / nw <= f32(1.0 / 256.0))) & (np.abs(u) <= f32(1) + REL + f32(1.0 / 256.0) * nu)
        kx, ky, kz = fx * tw[0] - tu[0], fx * tw[1] - tu[1], fx * tw[2] - tu[2]
        lx, ly, lz = fy * tw[0] - tv[0], fy * tw[1] - tv[1], fy * tw[2] - tv[2]
        p0, p1, p2 = ky * lz - kz * ly, kz * lx - kx * lz, kx * ly - ky * lx
        keep = inside & (p2 != f32(0))
        amb = np.abs(p2) <= REL * (np.abs(kx * ly) + np.abs(ky * lx))
        sx, sy = p0 / p2, p1 / p2
        rho3d = sx * sx + sy * sy
        ddx, ddy = qc[0] - fx, qc[1] - fy
        rho2d = f32(2.0) * (ddx * ddx + ddy * ddy)
        if "rho2d_dropped" in mut:
            rho2d = np.full_like(rho2d, np.inf)
        first = rho3d <= rho2d
        amb |= np.isfinite(rho2d) & (np.abs(rho3d - rho2d) <= REL * np.maximum(rho3d, rho2d))
        rho = np.where(rho3d < rho2d, rho3d, rho2d) if "min_is_rho3d" not in mut else rho3d
        depth = np.where(first, (sx * tw[0] + sy * tw[1]) + tw[2], np.full_like(rho, tw[2]))
        if "near_removed" not in mut:
            keep &= ~(depth < f32(0.2))
            amb |= np.abs(depth - f32(0.2)) <= REL * f32(0.2)
        power = f32(-0.5) * rho
        keep &= ~(power > f32(0))
        a0 = opa * np.exp(power)
        alpha = np.where(a0 > f32(0.99), f32(0.99), a0) if "cap_removed" not in mut else a0
        keep &= alpha >= f32(1.0) / f32(255.0)
        amb |= np.abs(alpha - f32(1.0) / f32(255.0)) <= REL * (f32(1.0) / f32(255.0))
        if dest_depth is not None:
            zs, dz = v["zwin"][i], dest_depth[ys, xs].astype(f32)
            if depth_unorm24:
                zs = f32(np.floor(np.float64(zs) * 16777215.0 + 0.5))
                dz = np.floor(dz.astype(np.float64) * 16777215.0 + 0.5).astype(f32)
            keep &= zs <= dz
            amb |= np.abs(zs - dz) <= REL * np.abs(dz)
        return np.where(keep, alpha, f32(0)).astype(f32), (amb & inside) | near_edge


def walk(v, order_far_to_near, width, height, mut=(), dest_depth=None, depth_unorm24=False):
    """Per drawn splat, near -> far: (index, ys, xs, alpha [h, w] over its pixel rect).  + the frame's ambiguous mask and covered mask."""
    amb = np.zeros((height, width), bool)
    cov = np.zeros((height, width), bool)
    frs = []
    for i in np.asarray(order_far_to_near)[::-1]:
        if not v["visible"][i]:
            continue
        x0, y0, x1, y1 = v["pixel_rect"][i]
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        a, am = fragments(v, i, xs, ys, mut, dest_depth, depth_unorm24)
        amb[y0:y1 + 1, x0:x1 + 1] |= am
        cov[y0:y1 + 1, x0:x1 + 1] |= (a > 0) | am
        frs.append((int(i), slice(y0, y1 + 1), slice(x0, x1 + 1), a))
    return frs, amb, cov


def _rgb_of(v, i):
    c0, c1 = int(v["c0"][i]), int(v["c1"][i])
    k = f32(1.0) / f32(65535.0)
    return f32(c0 & 0xFFFF) * k, f32(c0 >> 16) * k, f32(c1 & 0xFFFF) * k


def _round8(x):
    return (np.clip(x, f32(0), f32(1)) * f32(255.0) + f32(0.5)).astype(np.uint8)


def composite_fp32(v, frs, width, height, dest_rgba=None):
    """Front to back in fp32, rounded once: uint8 [h, w, 4] (row 0 = bottom), and the unrounded float frame."""
    T = np.ones((height, width), f32)
    C = np.zeros((height, width, 3), f32)
    for i, sy, sx, a in frs:
        w = T[sy, sx] * a
        for ch, col in enumerate(_rgb_of(v, i)):
            C[sy, sx, ch] = C[sy, sx, ch] + w * col
        T[sy, sx] = T[sy, sx] * (f32(1.0) - a)
    out = np.concatenate([C, (f32(1.0) - T)[..., None]], axis=2)
    if dest_rgba is not None:
        d = dest_rgba.astype(f32) * (f32(1.0) / f32(255.0))
        out = T[..., None] * d + out
    return _round8(out), out


def composite_rop8(v, frs, width, height, dest_rgba=None):
    """Back to front into an RGBA8 target, every channel rounded to 8 bits after every splat (floor(x * 255 + 0.5))."""
    fb = np.zeros((height, width, 4), f32) if dest_rgba is None else dest_rgba.astype(f32) * (f32(1.0) / f32(255.0))
    for i, sy, sx, a in frs[::-1]:
        hit = a > 0
        src = np.array([*_rgb_of(v, i), 1.0], f32)
        cur = fb[sy, sx]
        new = a[..., None] * src + (f32(1.0) - a[..., None]) * cur
        new = _round8(new).astype(f32) * (f32(1.0) / f32(255.0))
        fb[sy, sx] = np.where(hit[..., None], new, cur)
    return _round8(fb)


def render(case, order_far_to_near, mut=(), dest_depth=None, depth_unorm24=False, dest_rgba=None):
    """-> dict(frame uint8 [h, w, 4], exact float frame, ambiguous, covered, vertex outputs)."""
    v = vertex(case, mut)
    frs, amb, cov = walk(v, order_far_to_near, case["width"], case["height"], mut, dest_depth, depth_unorm24)
    frame, exact = composite_fp32(v, frs, case["width"], case["height"], dest_rgba)
    return dict(frame=frame, exact=exact, ambiguous=amb, covered=cov, vertex=v, fragments=frs)


def depth_order(case):
    """Indexes far -> near by view depth of the centre (a stable stand-in for the sorter: ties by index)."""
    c = case["centers"].astype(np.float64)
    mv = case["view"].astype(np.float64)
    zv = mv[2] * c[:, 0] + mv[6] * c[:, 1] + mv[10] * c[:, 2] + mv[14]
    return np.argsort(zv, kind="stable").astype(np.uint32)          # view z is negative in front: most negative = farthest first
