"""Seeded cases for the strip and block culls (test_strip_cull_ref.py on the CPU, test_gpu_strip_cull.py on the device): the
geometries where the hand-derived bounds of csrc/project.hip are tight, at the smallest size that still has many storage blocks.

Every case is a scene of 4 000 - 20 000 splats (never a multiple of 256; `needles` ends in a block of a single splat), a camera with a
320 x 200 viewport (13 tile rows, the last one partial) and the mesh options of one shader permutation.  The same camera looks at
the same slab in most of them, so what differs between two cases is the one thing the case is named for.
"""
from types import SimpleNamespace

import numpy as np

import strip_cull_ref as ref
from gaussiansplats3d_amd import camera

W, H = 320, 200
ROWS = (H + 15) // 16                                             # 13
CUTS = [(0, 1), (1, 6), (6, 7), (7, 12), (12, 13)]
STRIPS = [(r, r + 1) for r in range(ROWS)] + [c for c in CUTS if c[1] - c[0] > 1]
SETTINGS = {"default": None, "no_block_cull": "GSPLAT_NO_BLOCK_CULL", "no_block_list": "GSPLAT_NO_BLOCK_LIST",
            "block_test_always": "GSPLAT_BLOCK_TEST_ALWAYS"}
EYE, LOOK, UP = (0.0, 0.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)

NAMES = ["needles", "near_plane", "cap_default", "cap_small", "scale_small", "scale_large_focal2", "scale_8_tiny", "antialiased",
         "point_cloud", "half_cov", "specials_roll45_cap8", "roll90", "roll45", "inside", "along_axis", "orthographic", "mesh_world",
         "far_centres", "far_mesh_world", "dynamic", "straddle", "reupload", "scale_8_roll45", "big_round"]
SORTER_NAMES = ["needles", "half_cov"]                             # the two cases that also run through the visibility-culled sort


# -- building blocks ----------------------------------------------------------------------------------------------------------------
def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.empty((n, 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def covariances(rng, scales):
    """R diag(scales^2) R' with a random rotation per splat, as the six upper-triangle values."""
    scales = np.asarray(scales, dtype=np.float64)
    M = rotations(rng, scales.shape[0]) * scales[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)


def slab(rng, n, half=(5.0, 3.5, 2.0)):
    """Centres in a slab around the origin: from EYE it fills the frame and a margin around it, 4 to 8 units deep."""
    return (rng.uniform(-1.0, 1.0, size=(n, 3)) * np.asarray(half)).astype(np.float32)


def blobs(rng, n, sigma=0.03, spread=0.8):
    return covariances(rng, np.exp(rng.normal(np.log(sigma), spread, size=(n, 3))))


def colours(rng, n):
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    rgba[:, 3] = np.clip(rgba[:, 3], 8, 255)
    return rgba


def matrix(rot=None, scale=(1.0, 1.0, 1.0), translate=(0.0, 0.0, 0.0)):
    """Column-major 16-vector of translate * rot * diag(scale)."""
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) if rot is None else rot) * np.asarray(scale, dtype=np.float64)[None, :]
    m[:3, 3] = translate
    return np.ascontiguousarray(m.T).reshape(16)


def rot_zyx(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rz = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    ry = np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    rx = np.array([[1.0, 0, 0], [0, cc, -sc], [0, sc, cc]])
    return rz @ ry @ rx


def apply(m16, pts):
    m = np.asarray(m16, dtype=np.float64).reshape(4, 4).T
    return np.asarray(pts, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]


def morton_positions(centers, uploads):
    """Host restatement of the storage order (k_morton_keys + a stable sort per first upload of a range): position of every
    original index.  The CPU tier uses it to form storage blocks; the device tests read the real positions instead."""
    c = np.asarray(centers, dtype=np.float32)
    pos = np.empty(c.shape[0], dtype=np.int64)
    for lo, hi in uploads:
        seg = c[lo:hi]
        with np.errstate(all="ignore"):
            mn = np.array([np.min(seg[:, k][~np.isnan(seg[:, k])], initial=np.inf) for k in range(3)], dtype=np.float32)
            mx = np.array([np.max(seg[:, k][~np.isnan(seg[:, k])], initial=-np.inf) for k in range(3)], dtype=np.float32)
            inv = np.where(mx > mn, np.float32(1.0) / (mx - mn), np.float32(0.0)).astype(np.float32)
            t = (seg - mn) * inv * np.float32(1023.0)
            t = np.where(t < 0, 0.0, np.where(t > 1023.0, 1023.0, t))
        g = np.nan_to_num(t, nan=0.0).astype(np.uint32)

        def spread(v):
            v = (v | (v << 16)) & 0x030000FF
            v = (v | (v << 8)) & 0x0300F00F
            v = (v | (v << 4)) & 0x030C30C3
            return (v | (v << 2)) & 0x09249249
        key = spread(g[:, 0]) | (spread(g[:, 1]) << 1) | (spread(g[:, 2]) << 2)
        order = np.argsort(key, kind="stable")
        pos[lo + order] = lo + np.arange(hi - lo)
    return pos


def presorted(centers):
    """The centres in the storage order they would get on their own.  A non-finite centre makes the Morton bounds infinite and every
    key equal, so the storage keeps the upload order: uploading in this order keeps the blocks of such a scene compact."""
    out = np.empty_like(centers)
    out[morton_positions(centers, [(0, centers.shape[0])])] = centers
    return out


# -- the cases ----------------------------------------------------------------------------------------------------------------------
def make_case(name):
    rng = np.random.default_rng(7000 + NAMES.index(name))
    c = SimpleNamespace(name=name, cam=camera.PerspectiveCamera(W, H, EYE, LOOK, UP), mesh_kw={}, focal_adjustment=1.0, mesh_world=None,
                        scene_idx=None, transforms=None, uploads=None, reupload=None, half=False, block_strip=True)
    n = 12289                                                    # 48 blocks and one splat more
    if name == "needles":                                        # scale ratios up to 1 : 5000, any orientation
        n = 16385
        c.centers = slab(rng, n)
        long_ = np.exp(rng.uniform(np.log(0.02), np.log(0.25), size=n))
        ratio = np.exp(rng.uniform(0.0, np.log(5000.0), size=(n, 2)))
        ratio[: n // 3, 0] = 1.0                                  # a third are discs, the others needles
        c.cov = covariances(rng, np.stack([long_, long_ / ratio[:, 0], long_ / ratio[:, 1]], axis=1))
    elif name == "near_plane":                                   # depth 0.08 (in front of the near plane) .. 0.5, out to 1.3 x the frustum
        n = 16385 + 100
        depth = rng.uniform(0.08, 0.5, size=n)
        tan_y = np.tan(np.deg2rad(25.0))
        xy = rng.uniform(-1.3, 1.3, size=(n, 2)) * np.array([tan_y * W / H, tan_y]) * depth[:, None]
        c.centers = np.stack([xy[:, 0], xy[:, 1], EYE[2] - depth], axis=1).astype(np.float32)
        c.cov = covariances(rng, np.exp(rng.normal(np.log(0.005), 0.6, size=(n, 3))) * depth[:, None])
    elif name == "cap_default":                                  # a tight cluster of splats wider than 1024 px among small ones
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        big = np.arange(300)
        c.centers[big] = (np.array([-2.0, -1.5, 2.5]) + rng.normal(size=(300, 3)) * 0.05).astype(np.float32)
        c.cov[big] = covariances(rng, rng.uniform(6.0, 12.0, size=(300, 3)))
    elif name == "cap_small":                                    # maxScreenSpaceSplatSize 8: nearly every splat is clamped
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n, sigma=0.4, spread=0.5)
        c.mesh_kw = dict(max_screen_space_splat_size=8.0)
    elif name == "scale_small":
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n, sigma=0.1)
        c.mesh_kw = dict(splat_scale=0.3)
    elif name == "scale_large_focal2":
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n, sigma=0.01)
        c.mesh_kw = dict(splat_scale=3.0, kernel_2d_size=0.1)
        c.focal_adjustment = 2.0
    elif name == "scale_8_tiny":                                 # sub-pixel splats drawn 8 x: the floored discriminant decides the extent
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n, sigma=0.0015, spread=0.3)
        c.mesh_kw = dict(splat_scale=8.0, kernel_2d_size=0.32)
    elif name == "antialiased":
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        c.mesh_kw = dict(antialiased=True, kernel_2d_size=0.3)
    elif name == "point_cloud":
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n, sigma=0.005, spread=0.3)
        c.mesh_kw = dict(point_cloud_mode=True, splat_scale=6.0)          # (sqrt(8 * 0.2) = 1.26 px at scale 1: nothing would reach 4 px)
    elif name == "half_cov":                                     # halves rounded to nearest (half of them up), one overflow to inf, NaN
        c.centers = presorted(slab(rng, n))
        cov = blobs(rng, n, sigma=0.035, spread=0.5)
        cov[4001, [0, 3, 5]] = 70000.0                            # -> +inf in half
        cov[977::3001] = np.nan                                   # four splats in as many blocks
        cov[500::4001, 2] = np.nan                                # one value of the six
        c.centers[300::4099, 0] = np.nan
        c.centers[301::4099, 1] = np.inf
        c.centers[302::4099] = -np.inf
        with np.errstate(over="ignore"):
            h = cov.astype(np.float16)
        assert (h.astype(np.float32) > cov).sum() > n and np.isinf(h[4001, 0])
        c.cov = h.view(np.uint16)
        c.half = True
        c.mesh_kw = dict(half_precision_covariances=True)
    elif name == "specials_roll45_cap8":                         # NaN / inf centres and NaN covariances under the tightest reach
        c.cam = camera.PerspectiveCamera(W, H, (-1.5, 1.0, 6.0), LOOK, (1.0, 1.0, 0.2))   # no axis of the view is an axis of the world
        c.centers = presorted(slab(rng, n, half=(5.0, 5.0, 2.0)))
        c.cov = blobs(rng, n, sigma=0.08)
        c.cov[977::977] = np.nan
        c.centers[300::1400, 0] = np.nan                          # (1400 = 5.5 blocks: every kind in blocks of its own)
        c.centers[600::1400, 0] = np.inf
        c.centers[900::1400, 1] = -np.inf
        c.centers[1200::2800, 2] = np.inf
        c.centers[1500::2800] = np.nan
        c.mesh_kw = dict(max_screen_space_splat_size=8.0)
    elif name in ("roll90", "roll45"):
        c.cam = camera.PerspectiveCamera(W, H, EYE, LOOK, (1.0, 0.0, 0.0) if name == "roll90" else (1.0, 1.0, 0.0))
        c.centers = slab(rng, n, half=(3.5, 5.0, 2.0) if name == "roll90" else (5.0, 5.0, 2.0))
        c.cov = blobs(rng, n, sigma=0.045, spread=0.5)
    elif name == "inside":
        n = 19969
        c.cam = camera.PerspectiveCamera(W, H, (0.3, 0.2, 0.1), (3.0, 1.0, 2.0), (0.0, -1.0, 0.0))
        c.centers = slab(rng, n, half=(5.0, 3.5, 3.5))                # all around the camera, and most of it where it looks
        fwd = (np.array([3.0, 1.0, 2.0]) - c.cam.position) / np.linalg.norm(np.array([3.0, 1.0, 2.0]) - c.cam.position)
        c.centers[n // 4:] = (slab(rng, n - n // 4, half=(2.5, 2.5, 2.5)) + c.cam.position + 4.5 * fwd).astype(np.float32)
        dist = np.linalg.norm(c.centers - np.asarray(c.cam.position), axis=1)             # a few pixels wide at any depth
        c.cov = covariances(rng, np.exp(rng.normal(np.log(0.006), 0.5, size=(n, 3))) * dist[:, None])
    elif name == "along_axis":                                   # looking straight down the world's up axis (lookAt's degenerate branch)
        c.cam = camera.PerspectiveCamera(W, H, (0.0, 6.0, 0.0), LOOK, UP)
        c.centers = slab(rng, n, half=(5.0, 2.0, 5.0))
        c.cov = blobs(rng, n)
    elif name == "orthographic":
        c.cam = camera.OrthographicCamera(W, H, EYE, LOOK, UP, zoom=30.0)
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        c.block_strip = False                                     # the block strip test stands down, the pre-test takes the zoom branch
    elif name == "mesh_world":                                   # non-uniform scale and a rotation in the mesh's transform
        c.mesh_world = matrix(rot_zyx(0.5, -0.4, 0.3), scale=(0.2, 1.0, 5.0), translate=(0.3, -0.2, 0.1))
        world = slab(rng, n)
        c.centers = apply(np.linalg.inv(c.mesh_world.reshape(4, 4).T).T.reshape(16), world).astype(np.float32)
        c.cov = blobs(rng, n, sigma=0.012, spread=0.4)
    elif name in ("far_centres", "far_mesh_world"):              # the scene 1000 units from the origin
        off = np.array([600.0, -500.0, 624.0])
        c.cam = camera.PerspectiveCamera(W, H, tuple(off + EYE), tuple(off + LOOK), UP)
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        if name == "far_centres":
            c.centers = (c.centers.astype(np.float64) + off).astype(np.float32)
        else:
            c.mesh_world = matrix(translate=off)
    elif name == "dynamic":                                      # three scenes, one scaled x 4: no block cull, the pre-test has only the cap
        world = slab(rng, n)
        c.scene_idx = (np.arange(n) % 3).astype(np.uint32)
        c.transforms = [matrix(), matrix(rot_zyx(0.3, 0.2, -0.1), translate=(0.4, -0.2, 0.1)), matrix(scale=(4.0, 4.0, 4.0), translate=(-0.5, 0.3, 0.0))]
        local = np.empty((n, 3))
        for s, t in enumerate(c.transforms):
            sel = c.scene_idx == s
            local[sel] = apply(np.linalg.inv(t.reshape(4, 4).T).T.reshape(16), world[sel])
        c.centers = local.astype(np.float32)
        c.cov = blobs(rng, n, sigma=0.02)
        c.mesh_kw = dict(dynamic_mode=True, max_screen_space_splat_size=8.0)
        c.block_strip = False
    elif name == "straddle":                                     # the first upload is one storage block on both sides of the camera plane
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        c.centers[:256] = np.stack([rng.uniform(-0.5, 0.5, 256), rng.uniform(-0.4, 0.4, 256), EYE[2] + rng.uniform(-1.0, 1.0, 256)],
                                   axis=1).astype(np.float32)
        c.cov[:256] = blobs(rng, 256, sigma=0.004)
        c.uploads = [(0, 256), (256, n)]
    elif name == "reupload":                                     # a sub-range mirrored to the other side of the frame after the first upload
        c.centers = slab(rng, n)
        c.cov = blobs(rng, n)
        lo, hi = 3000, 5500
        c.centers[lo:hi, 1] = np.abs(c.centers[lo:hi, 1]) * 0.5 + 1.0            # all of it in the upper half ...
        moved = c.centers[lo:hi].copy()
        moved[:, 1] = -moved[:, 1]                                                  # ... then in the lower one
        c.reupload = (lo, hi, moved)
    elif name == "scale_8_roll45":                               # scale_8_tiny again, seen by a rolled camera off the axis
        c.cam = camera.PerspectiveCamera(W, H, (-1.5, 1.0, 6.0), LOOK, (1.0, 1.0, 0.2))
        c.centers = slab(rng, n, half=(5.0, 5.0, 2.0))
        c.cov = blobs(rng, n, sigma=0.0015, spread=0.3)
        c.mesh_kw = dict(splat_scale=8.0, kernel_2d_size=0.32)
    elif name == "big_round":                                    # spheres ~ 7 px in sigma: Gershgorin is exact, so all of the extent
        c.centers = slab(rng, n)                                 # beyond j11 comes from row 2 of mat3(modelView), most off the axis
        s2 = np.exp(rng.normal(np.log(0.2), 0.15, size=n)) ** 2
        c.cov = np.stack([s2, 0 * s2, 0 * s2, s2, 0 * s2, s2], axis=1).astype(np.float32)
    else:
        raise KeyError(name)
    c.count = c.centers.shape[0]
    assert 4000 <= c.count <= 20000 and c.count % 256 != 0
    c.rgba = colours(rng, c.count)
    c.uploads = c.uploads or [(0, c.count)]
    return c


def final_centers(case):
    """The centres the mesh holds when it is drawn (after the re-upload, if the case has one)."""
    out = case.centers.copy()
    if case.reupload:
        lo, hi, moved = case.reupload
        out[lo:hi] = moved
    return out


def cov_read(case):
    """The covariance values the shader reads: fp32 as uploaded, or the halves widened."""
    return case.cov.view(np.float16).astype(np.float32) if case.half else case.cov


def model_uniforms(case):
    kw = case.mesh_kw
    return ref.uniforms(case.cam, focal_adjustment=case.focal_adjustment, mesh_world=case.mesh_world, splat_scale=kw.get("splat_scale", 1.0),
                        kernel2d=kw.get("kernel_2d_size", 0.3), max_splat_px=kw.get("max_screen_space_splat_size", 1024.0),
                        antialiased=kw.get("antialiased", False), point_cloud=kw.get("point_cloud_mode", False),
                        dynamic=kw.get("dynamic_mode", False))


def splat_views(case, u):
    """One modelView per splat for per-scene transforms (viewMatrix * transform, in the kernel's fp32 inputs), else None."""
    if case.transforms is None:
        return None
    return ref.scene_views(u.view_matrix, case.transforms)[case.scene_idx]


def build_mesh(ctx, case, setting="default"):
    """The case's mesh on the device, drawn in upload order: created under the setting's switch (read at mesh creation), uploaded
    in the case's segments, re-uploaded if the case says so, camera set.  max_splat_count is the case's count, so the last storage
    block holds the case's splats only."""
    import os

    from gaussiansplats3d_amd import SplatMesh
    env = SETTINGS[setting]
    if env:
        os.environ[env] = "1"
    try:
        mesh = SplatMesh(ctx, case.count, 0, **case.mesh_kw)
    finally:
        if env:
            del os.environ[env]

    def upload(lo, hi, centers):
        mesh.build(centers, case.cov[lo:hi], case.rgba[lo:hi], None, start=lo,
                   scene_indexes=None if case.scene_idx is None else case.scene_idx[lo:hi], covariances_are_half_bits=case.half)
    for lo, hi in case.uploads:
        upload(lo, hi, case.centers[lo:hi])
    if case.transforms is not None:
        mesh.set_scenes(transforms=case.transforms, camera_position=case.cam.position)
    if case.reupload:
        lo, hi, moved = case.reupload
        upload(lo, hi, moved)
    mesh.set_camera(case.cam, focal_adjustment=case.focal_adjustment, mesh_world=case.mesh_world)
    mesh.update_render_indexes(np.arange(case.count, dtype=np.uint32), case.count)
    return mesh
