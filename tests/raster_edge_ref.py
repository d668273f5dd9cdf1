"""The vertex stage's ACCEPT / REJECT chain restated in numpy float32, one rounding per operation, in the order the reference's
shader states it (SplatMaterial.js:123-166, SplatMaterial3D.js:83-210): nothing but the quantities a verdict depends on.  Colour,
spherical harmonics and the fade never decide whether a splat is drawn and are not here.

tests/test_raster_edge_ref.py holds verdicts() to the shader's own verdicts on every splat of tests/raster_edge_cases.py - the
knife-edge covariances included, where the last bit of `traceOver2 * traceOver2 - D` decides - and then MUTATES it (`mut` below):
each mutation must change a verdict of a named class, which proves that the cases can see that mistake in the kernel.
tests/raster_edge_cases.py also asks it where a threshold lies between two adjacent floats, to place its ladders there; what the
ladders then prove is counted on the shader's outputs alone (the census of the golden file).

mut: a dict, every key optional -
  "swap": a set of comparison names whose strictness is swapped (`>` <-> `>=`, `<` <-> `<=`): "x_hi", "x_lo", "y_hi", "y_lo", "z_plane",
          "z_near", "z_far", "opacity", "aa", "eig2"
  "ulp":  {constant name: +1 / -1}: "1.2", "0.1", "0.01" moved by one ulp
  "fused_disc": traceOver2 * traceOver2 - D with one rounding;  "split_trace": 0.5 * a + 0.5 * d;  "no_nan_check";  "no_z_test"."""
import numpy as np

F = np.float32


def _const(mut, name):
    v = F(float(name))
    k = mut.get("ulp", {}).get(name, 0)
    return (v.view(np.uint32) + np.uint32(k)).view(F) if k >= 0 else (v.view(np.uint32) - np.uint32(-k)).view(F)


def _lt(mut, name, a, b):
    return a <= b if name in mut.get("swap", ()) else a < b


def _gt(mut, name, a, b):
    return a >= b if name in mut.get("swap", ()) else a > b


def _le(mut, name, a, b):
    return a < b if name in mut.get("swap", ()) else a <= b


def _ge(mut, name, a, b):
    return a > b if name in mut.get("swap", ()) else a >= b


def _f32(m):
    return np.asarray(m, np.float64).astype(F).reshape(-1)


def verdicts(case, mut=None, centers=None, cov=None, rgba=None, scene_idx=None, capped=False):
    """drawn [n] bool and the stage flags {plane, scene, z, aa, eig2, nan} (each: rejected THERE, having passed everything before) of a
    raster case's splats - or of other splats (centers / cov / rgba / scene_idx) under the case's uniforms and switches.
    capped=True: instead of `drawn`, whether min(sqrt8 * sqrt(eigenValue1), maxScreenSpaceSplatSize) takes the cap - no decision (the
    minimum is continuous), but the float at which a footprint stops growing."""
    mut = mut or {}
    u = case["uniforms"]
    dynamic, effects = case["dynamic"], case["effects"]
    c = np.asarray(case["centers"] if centers is None else centers, F)
    V = np.asarray(case["cov"] if cov is None else cov, F)
    byte = np.asarray(case["rgba"] if rgba is None else rgba)[:, 3]
    n = c.shape[0]
    of = case["scene_idx"] if scene_idx is None else scene_idx
    scene = np.zeros(n, np.int64) if (of is None or u["scene_count"] <= 1) else np.asarray(of, np.int64)
    with np.errstate(all="ignore"):
        scene_ok = np.ones(n, bool)
        if effects:                                                                     # SplatMaterial.js:129-137
            opacity = np.asarray(u["scene_opacity"], F)[scene]
            visible = np.asarray(u["scene_visibility"], np.int64)[scene]
            scene_ok = ~(_le(mut, "opacity", opacity, _const(mut, "0.01")) | (visible == 0))
        if dynamic:                                                                     # :140-144 viewMatrix * transform
            A = _f32(u["view_matrix"])
            per_scene = []
            for t in u["transforms"]:
                B = _f32(t)
                per_scene.append([A[r] * B[4 * col] + A[4 + r] * B[4 * col + 1] + A[8 + r] * B[4 * col + 2] + A[12 + r] * B[4 * col + 3]
                                  for col in range(4) for r in range(4)])
            MV = np.asarray(per_scene, F)[scene].T                                       # [16, n]
        else:
            MV = np.repeat(_f32(u["model_view"])[:, None], n, axis=1)
        P = _f32(u["projection"])
        c0, c1, c2 = c[:, 0], c[:, 1], c[:, 2]
        v = [MV[r] * c0 + MV[4 + r] * c1 + MV[8 + r] * c2 + MV[12 + r] for r in range(4)]      # :156
        q = [P[r] * v[0] + P[4 + r] * v[1] + P[8 + r] * v[2] + P[12 + r] * v[3] for r in range(4)]   # :158
        clip = _const(mut, "1.2") * q[3]                                                 # :160-164
        plane = (_lt(mut, "z_plane", q[2], -clip) | _lt(mut, "x_lo", q[0], -clip) | _gt(mut, "x_hi", q[0], clip) |
                 _lt(mut, "y_lo", q[1], -clip) | _gt(mut, "y_hi", q[1], clip))
        ndcx, ndcy, ndcz = q[0] / q[3], q[1] / q[3], q[2] / q[3]                         # :166
        z_ok = _ge(mut, "z_near", ndcz, F(-1.0)) & _le(mut, "z_far", ndcz, F(1.0))       # GL clips the quad at its centre's depth
        if "no_z_test" in mut:
            z_ok = np.ones(n, bool)
        alpha = byte.astype(F) * (F(1.0) / F(255.0))
        # SplatMaterial3D.js:111-134
        if u["orthographic"]:
            j00 = j11 = np.full(n, F(u["ortho_zoom"]))
            j20 = j21 = np.zeros(n, F)
        else:
            s = F(1.0) / (v[2] * v[2])
            fx, fy = F(u["focal"][0]), F(u["focal"][1])
            j00, j20 = fx / v[2], -(fx * v[0]) * s
            j11, j21 = fy / v[2], -(fy * v[1]) * s
        T0 = [MV[4 * r + 0] * j00 + MV[4 * r + 2] * j20 for r in range(3)]
        T1 = [MV[4 * r + 1] * j11 + MV[4 * r + 2] * j21 for r in range(3)]
        V00, V01, V02, V11, V12, V22 = (V[:, k] for k in range(6))

        def times_v(T):
            return [V00 * T[0] + V01 * T[1] + V02 * T[2], V01 * T[0] + V11 * T[1] + V12 * T[2], V02 * T[0] + V12 * T[1] + V22 * T[2]]
        VT0, VT1 = times_v(T0), times_v(T1)
        a = T0[0] * VT0[0] + T0[1] * VT0[1] + T0[2] * VT0[2]
        b = T0[0] * VT1[0] + T0[1] * VT1[1] + T0[2] * VT1[2]
        d = T1[0] * VT1[0] + T1[1] * VT1[1] + T1[2] * VT1[2]
        kernel = F(case["kernel2d"])
        aa_ok = np.ones(n, bool)
        if case["antialiased"]:                                                          # :137-144
            det0 = a * d - b * b
            a, d = a + kernel, d + kernel
            det1 = a * d - b * b
            ratio = det0 / det1
            alpha = alpha * np.sqrt(np.where(ratio < 0, F(0.0), ratio))                  # max(x, 0.0): 0 only where x < 0
            aa_ok = ~_lt(mut, "aa", alpha, F(1.0) / F(255.0))
        else:
            a, d = a + kernel, d + kernel
        D = a * d - b * b                                                                # :174-188
        half_tr = (F(0.5) * a + F(0.5) * d) if "split_trace" in mut else F(0.5) * (a + d)
        if "fused_disc" in mut:
            disc = (half_tr.astype(np.float64) * half_tr.astype(np.float64) - D.astype(np.float64)).astype(F)
        else:
            disc = half_tr * half_tr - D
        floor = _const(mut, "0.1")
        term2 = np.sqrt(np.where(floor < disc, disc, floor))                             # max(0.1, x): x only where 0.1 < x
        l1, l2 = half_tr + term2, half_tr - term2
        if u["point_cloud"]:
            l1 = l2 = np.full(n, F(0.2))
        eig_ok = ~_le(mut, "eig2", l2, F(0.0))
        ex, ey = b, l1 - a                                                               # :190
        elen = np.sqrt(ex * ex + ey * ey)
        e1x, e1y = ex / elen, ey / elen
        cap = F(case["max_splat_px"])
        sqrt8 = np.sqrt(F(8.0))
        h1, h2 = sqrt8 * np.sqrt(l1), sqrt8 * np.sqrt(l2)
        at_cap = cap < h1
        h1, h2 = np.where(cap < h1, cap, h1), np.where(cap < h2, cap, h2)                # min(x, cap): cap only where cap < x
        finite = np.isfinite(ndcx) & np.isfinite(ndcy) & np.isfinite(ndcz) & np.isfinite(e1x * h1) & np.isfinite(e1y * h1) & \
            np.isfinite(e1x * h2) & np.isfinite(e1y * h2)
        if "no_nan_check" in mut:
            finite = np.ones(n, bool)
    stages = {}
    alive = np.ones(n, bool)
    for name, ok in (("scene", scene_ok), ("plane", ~plane), ("z", z_ok), ("aa", aa_ok), ("eig2", eig_ok), ("nan", finite)):
        stages[name] = alive & ~ok
        alive = alive & ok
    return (at_cap if capped else alive), stages
