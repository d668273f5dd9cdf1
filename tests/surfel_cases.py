"""Seeded inputs of the SplatRenderMode.TwoD tests: shared by tests/test_surfel_ref.py (the host model alone, CPU) and
tests/test_gpu_surfel.py (the HIP vertex stage and blend against the model).  The smallest shapes at which the two kernels can go
wrong: both quad branches, splats behind the camera / beyond the far plane / edge-on, every shader permutation of the base stage,
lists around the blend's batch size of 256, quads on quadrant, bin and frame borders.

Whoever changes the 2D fragment chain extends these cases and the mutations of tests/surfel_ref.py."""
import functools

import numpy as np

import surfel_ref
from gaussiansplats3d_amd import camera

AMBIGUOUS_CAP = 0.01          # every frame case: at most 1 % of its covered pixels may be ambiguous


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1.0                                     # (x, y, z, w), w >= 0 as fillSplatScaleRotationArray leaves it
    return q.astype(np.float32)


def surfel_scene(n, seed, scale=0.02, sigma=1.0, cam=None, extremes=True):
    """Surfels in a slab in front of the garden camera; scales straddle one pixel so that both quad branches occur, a few splats sit
    beyond the far plane (the cameras here end at 12), behind the camera, and edge-on through the eye."""
    rng = np.random.default_rng(seed)
    up, pos, look = (np.array(a) for a in camera.DEMO_POSES["garden"])
    fwd = (look - pos) / np.linalg.norm(look - pos)
    centers = pos + fwd * rng.uniform(0.4, 9.0, size=(n, 1)) + rng.normal(size=(n, 3)) * 1.0
    scales = np.exp(rng.normal(np.log(scale), sigma, size=(n, 3)))
    rot = _quats(rng, n)
    if extremes:
        centers[0:8] = pos + fwd * rng.uniform(13.0, 30.0, size=(8, 1)) + rng.normal(size=(8, 3)) * 0.5     # beyond far
        centers[8:16] = pos - fwd * rng.uniform(0.5, 3.0, size=(8, 1)) + rng.normal(size=(8, 3)) * 0.2      # behind the camera
        for k in range(16, 28):                                # edge-on: the surfel's plane holds the eye, its normal is
            d = centers[k] - pos                               # perpendicular to the view ray
            d /= np.linalg.norm(d)
            nrm = np.cross(d, rng.normal(size=3))
            nrm /= np.linalg.norm(nrm)
            t1 = d
            t2 = np.cross(nrm, t1)
            R = np.stack([t1, t2, nrm], axis=1)                # columns: the surfel's two tangents and its normal
            w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
            w = max(w, 1e-3)
            q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
            rot[k] = (q / np.linalg.norm(q)).astype(np.float32)
            scales[k, :2] = scale * 0.2                        # small: the AABB branch, where |distance| < 1e-5 rejects
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    rgba[:, 3] = np.clip(rgba[:, 3], 1, 255)
    return centers.astype(np.float32), scales.astype(np.float32), rot, rgba


def _garden(w, h, far=12.0):
    up, pos, look = camera.DEMO_POSES["garden"]
    return camera.PerspectiveCamera(w, h, pos, look, up, far=far)


VERTEX_CASES = ["sh0", "sh2", "sh8", "effects", "dynamic", "fade_in", "orthographic", "focal_adjustment"]


@functools.lru_cache(maxsize=None)
def vertex_case(name):
    n, w, h = 2000, 512, 288
    cam = _garden(w, h)
    seed = 4100 + VERTEX_CASES.index(name)
    c, s, r, rgba = surfel_scene(n, seed)
    kw = {}
    if name in ("sh2", "sh8", "dynamic"):                      # SH-2 as the mesh stores it: fp16, or uint8 over (-0.9, 1.1)
        sh = np.random.default_rng(seed + 50).normal(0, 0.25, size=(n, 24)).astype(np.float16)
        kw = dict(sh=sh, sh_degree=2)
        if name == "sh8":
            sh8 = np.clip(np.floor((np.clip(sh.astype(np.float32), -0.9, 1.1) + 0.9) / 2.0 * 255.0), 0, 255).astype(np.uint8)
            kw = dict(sh=sh8, sh_degree=2, sh8_range=(-0.9, 1.1))
    if name == "effects":
        kw = dict(scene_idx=(np.arange(n) % 3).astype(np.uint32), opacity=[1.0, 0.4, 0.005], visible=[1, 0, 1])
    elif name == "dynamic":
        co, si = np.cos(0.3), np.sin(0.3)
        t1 = np.array([[co, 0, si, 0.4], [0, 1, 0, -0.2], [-si, 0, co, 0.1], [0, 0, 0, 1]]).T.reshape(16)
        kw.update(scene_idx=(np.arange(n) % 2).astype(np.uint32), transforms=[np.eye(4).T.reshape(16), t1])
    elif name == "fade_in":
        center = c.mean(axis=0)
        kw = dict(fade=(center.astype(np.float32).tolist(), float(np.median(np.linalg.norm(c - center, axis=1)))))
    elif name == "orthographic":
        up, pos, look = camera.DEMO_POSES["garden"]
        cam = camera.OrthographicCamera(w, h, pos, look, up, zoom=40.0, far=12.0)
        s = s * 2.0                                            # zoom 40 px per unit: scales straddle one pixel around 1 / 40
    elif name == "focal_adjustment":
        kw = dict(inv_focal_adj=0.5)
    return surfel_ref.make_case(c, s, r, rgba, cam, **kw)


FRAME_CASES = ["opaque", "translucent", "mixed_branches", "orthographic", "depth32f", "depth24"]


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """-> (case, order far -> near, destination kwargs for the model / the mesh).  Seeded until the model alone leaves at most
    AMBIGUOUS_CAP of the covered pixels ambiguous (the first seed of the case's own range that does)."""
    for seed in range(4200 + 100 * FRAME_CASES.index(name), 4300 + 100 * FRAME_CASES.index(name)):
        case, order, dest = _frame_case(name, seed)
        out = surfel_ref.render(case, order, **dest)
        if (out["ambiguous"] & out["covered"]).sum() <= AMBIGUOUS_CAP * out["covered"].sum():
            return case, order, dest
    raise AssertionError(f"no seed of frame case {name} stays under the ambiguous-pixel cap")


def _gap(zs, q):
    """A stored depth in the widest gap between splat depths near their quantile q: no splat's depth test is a near tie."""
    z = np.sort(zs.astype(np.float64))
    k = int(q * (z.size - 1))
    lo, hi = max(k - 12, 0), min(k + 12, z.size - 1)
    j = lo + int(np.argmax(np.diff(z[lo:hi + 1])))
    return np.float32(0.5 * (z[j] + z[j + 1]))


def _frame_case(name, seed):
    w, h, n = 160, 96, 180 if name == "orthographic" else 300
    cam = _garden(w, h)
    scale, sigma = 0.05, 0.7
    if name == "mixed_branches":
        scale, sigma = 0.012, 1.2
    c, s, r, rgba = surfel_scene(n, seed, scale, sigma)
    if name == "opaque":
        rgba[:, 3] = 255
    elif name == "translucent":
        rgba[:, 3] = np.random.default_rng(seed).integers(8, 90, n)
    elif name == "orthographic":
        up, pos, look = camera.DEMO_POSES["garden"]
        cam = camera.OrthographicCamera(w, h, pos, look, up, zoom=14.0, far=12.0)
        s = s * 5.0
    case = surfel_ref.make_case(c, s, r, rgba, cam)
    dest = {}
    if name in ("depth32f", "depth24"):
        v = surfel_ref.vertex(case)
        zs = v["zwin"][v["visible"]]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        depth = np.where(xx + yy < (w + h) / 2, _gap(zs, 0.3), _gap(zs, 0.5)).astype(np.float32)   # a step across the frame
        depth[: h // 5, : w // 5] = 1.0                          # a hole: nothing drawn there
        dst = np.random.default_rng(seed + 1).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        dst[..., 3] = np.where(depth < 1.0, 255, 0)
        dst[depth >= 1.0, :3] = 0
        dest = dict(dest_depth=depth, depth_unorm24=name == "depth24", dest_rgba=dst)
    return case, surfel_ref.depth_order(case), dest


# ---------------------------------------------------------------------------------------------------------------------------
# designed blend cases: a camera at the origin looking down -z, surfels placed by pixel
# ---------------------------------------------------------------------------------------------------------------------------
def _front_cam(w, h):
    return camera.PerspectiveCamera(w, h, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), far=50.0)


def _focal(h):
    return h / 2.0 / np.tan(np.radians(camera.THREE_FOV_DEG) / 2.0)


def _place(w, h, px, py, depth, basis_px, angle=0.0, tilt=0.0, aspect=1.0):
    """Centre, scale, rotation of a surfel whose centre projects to window position (px, py) at view depth `depth`, whose first
    basis vector is basis_px pixels long on screen (the second: aspect times that), rotated by `angle` in the image plane and
    tilted by `tilt` about its own first axis."""
    f = _focal(h)
    c = np.array([(px - w / 2.0) * depth / f, (py - h / 2.0) * depth / f, -depth])
    s = basis_px * depth / f
    ca, sa, ct, st = np.cos(angle / 2), np.sin(angle / 2), np.cos(tilt / 2), np.sin(tilt / 2)
    qz = np.array([0.0, 0.0, sa, ca])                          # about z by angle
    qx = np.array([st, 0.0, 0.0, ct])                          # then about the surfel's own x by tilt

    def mul(a, b):                                             # Hamilton product, (x, y, z, w)
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                         aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
    q = mul(qz, qx)
    if q[3] < 0:
        q = -q
    return c, np.array([s, s * aspect, 1.0]), q


DESIGNED_CASES = ["list_1", "list_255", "list_256", "list_257", "list_513", "one_quadrant", "quadrant_border", "bin_border",
                  "frame_edge", "long_rotated", "near_plane_crossing", "rho_balance", "basis_one_pixel", "termination",
                  "destination_between", "distance_reject"]


@functools.lru_cache(maxsize=None)
def designed_case(name):
    """-> (case, order far -> near, destination kwargs)."""
    w, h = (70, 50) if name in ("frame_edge", "long_rotated", "basis_one_pixel") else (64, 64)
    rng = np.random.default_rng(4300 + DESIGNED_CASES.index(name))
    items, dest = [], {}
    alpha = None
    if name.startswith("list_"):                               # that many entries on the one list of bin (0, 0), all reaching it
        count = int(name[5:])
        for k in range(count):                                 # (axis-aligned, edges a quarter pixel from every pixel centre)
            items.append(_place(w, h, rng.integers(6, 26) + 0.5, rng.integers(6, 26) + 0.5, 2.0 + 0.01 * k, (rng.integers(3, 6) + 0.25) / 3.0))
        alpha = rng.integers(2, 40, count)                     # translucent: nothing saturates, every entry is composited
    elif name == "one_quadrant":
        items = [_place(w, h, 40.3, 8.6, 2.0, 1.9, 0.4)]
    elif name == "quadrant_border":
        items = [_place(w, h, 16.2, 47.9, 2.0, 3.1, 0.9), _place(w, h, 47.6, 16.1, 2.5, 2.7, 0.2)]
    elif name == "bin_border":
        items = [_place(w, h, 31.7, 32.4, 2.0, 4.2, 1.1), _place(w, h, 32.0, 10.0, 3.0, 2.0, 0.0)]
    elif name == "frame_edge":                                 # over the right / top edge of a 70 x 50 frame
        items = [_place(w, h, 68.4, 25.0, 2.0, 3.0, 0.3), _place(w, h, 30.0, 49.2, 2.0, 3.3, 1.2), _place(w, h, 69.5, 49.5, 2.5, 2.0, 0.7)]
    elif name == "long_rotated":                               # its rect covers quadrants the quad never enters
        items = [_place(w, h, 33.3, 24.6, 2.0, 11.0, 0.7, aspect=0.1)]
    elif name == "near_plane_crossing":                        # the surfel's plane passes through depth 0.2 inside its quad
        items = [_place(w, h, 30.2, 33.1, 0.22, 9.0, 0.3, tilt=1.0)]
    elif name == "rho_balance":                                # AABB-branch surfels: rho2d (pixels) against rho3d across the quad
        items = [_place(w, h, 20.3, 20.7, 2.0, 0.7, 0.2), _place(w, h, 40.7, 41.3, 2.2, 0.9, 1.0, aspect=0.8)]
    elif name == "basis_one_pixel":                            # basis length just below and just above minPix
        items = [_place(w, h, 20.7, 20.3, 2.0, 0.999), _place(w, h, 45.7, 25.3, 2.0, 1.001),
                 _place(w, h, 30.7, 40.3, 2.0, 1.3, aspect=0.76), _place(w, h, 55.7, 40.3, 2.0, 1.3, aspect=0.78)]
    elif name == "termination":                                # three opaque surfels in front of 300
        for k in range(300):
            items.append(_place(w, h, rng.integers(8, 56) + 0.5, rng.integers(8, 56) + 0.5, 3.0 + 0.01 * k, (rng.integers(4, 12) + 0.25) / 3.0))
        for k in range(3):
            items.append(_place(w, h, 32.5 + k, 32.5 - k, 2.0 - 0.1 * k, (40 + k + 0.25) / 3.0))
        alpha = np.concatenate([rng.integers(100, 256, 300), [255, 255, 255]])
    elif name == "destination_between":
        items = [_place(w, h, 30.0, 30.0, 2.0, 5.0, 0.3), _place(w, h, 34.0, 33.0, 4.0, 6.0, 1.0)]
    elif name == "distance_reject":
        # a visible surfel, and one the AABB branch returns on (SplatMaterial2D.js:167, gl_Position unwritten): edge-on, its first
        # tangent (scale = its depth) reaching exactly the camera plane, so that Tw.z^2 - Tw.x^2 - Tw.y^2 is 0 within 1e-5
        items = [_place(w, h, 20.3, 40.6, 2.0, 2.2, 0.5),
                 (np.array([0.0, 0.0, -0.5]), np.array([0.5, 0.001, 1.0]), np.array([0.0, -np.sqrt(0.5), 0.0, np.sqrt(0.5)]))]
    else:
        raise KeyError(name)
    n = len(items)
    c = np.stack([i[0] for i in items])
    s = np.stack([i[1] for i in items])
    r = np.stack([i[2] for i in items])
    rgba = rng.integers(30, 256, size=(n, 4), dtype=np.uint8)
    rgba[:, 3] = 255 if alpha is None else alpha
    case = surfel_ref.make_case(c, s, r, rgba, _front_cam(w, h))
    if name == "destination_between":
        z = surfel_ref.vertex(case)["zwin"]
        depth = np.full((h, w), 0.5 * (float(z[0]) + float(z[1])), np.float32)      # between the two surfels
        depth[:, : w // 2] = 1.0
        dst = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        dest = dict(dest_depth=depth, depth_unorm24=False, dest_rgba=dst)
    return case, surfel_ref.depth_order(case), dest
