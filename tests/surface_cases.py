"""Scenes of the surface-pass tests (tests/test_surface_ref.py on the CPU, tests/test_gpu_surface.py on the device) and the glue
between a drawn mesh and the host model (surface_ref.py)."""
import numpy as np

import helpers
import surface_ref as ref
from gaussiansplats3d_amd import camera, scenes
from gaussiansplats3d_amd import _lib as L

K_POWER = float(np.float32(2.4022448))          # GS_K_POWER of csrc/project.hip


def small_camera(w=64, h=64):
    return camera.PerspectiveCamera(w, h, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))


def layer(cam, depth, radius_px, offset_px=(0.0, 0.0), count=1):
    """`count` coincident isotropic splats `depth` in front of `cam`, `offset_px` from the screen centre, about radius_px
    (sqrt(8) standard deviations) on screen: (centers [count, 3], cov [count, 6])."""
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    right, up, fwd = mw[0:3], mw[4:7], -mw[8:11]
    focal = cam.focal()[1]
    c = cam.position + fwd * depth + right * (offset_px[0] * depth / focal) + up * (offset_px[1] * depth / focal)
    s = (radius_px * depth / (np.sqrt(8.0) * focal)) ** 2
    return (np.tile(c.astype(np.float32), (count, 1)), np.tile(np.array([[s, 0, 0, s, 0, s]], np.float32), (count, 1)))


def scene_of(parts, alphas):
    """parts: (centers, cov) pairs; alphas: one 8-bit alpha per part."""
    centers = np.concatenate([p[0] for p in parts]).astype(np.float32)
    cov = np.concatenate([p[1] for p in parts]).astype(np.float32)
    rgba = np.full((centers.shape[0], 4), 200, dtype=np.uint8)
    rgba[:, 3] = np.concatenate([np.full(p[0].shape[0], a, dtype=np.uint8) for p, a in zip(parts, alphas)])
    return scenes.SplatScene(centers, cov, rgba, np.zeros((centers.shape[0], 0), np.float16), 0)


def one_opaque(cam, offset_px=(0.0, 0.0)):
    return scene_of([layer(cam, 4.0, 10.0, offset_px)], [255])


def two_layers(cam):
    """Two frame-filling layers of alpha 102 / 255 = 0.4: splat 0 near, splat 1 far."""
    return scene_of([layer(cam, 3.0, 1500.0), layer(cam, 5.0, 1500.0)], [102, 102])


def behind_the_eye(cam):
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    c = (cam.position + mw[8:11] * 2.0).astype(np.float32)[None, :]
    return scene_of([(c, np.array([[1e-2, 0, 0, 1e-2, 0, 1e-2]], np.float32))], [255])


def pile(cam, count):
    """`count` coincident frame-filling splats of 8-bit alpha 1 (drawn with a scene opacity: alpha = opacity / 255)."""
    return scene_of([layer(cam, 4.0, 1500.0, count=count)], [1])


def occluded(cam):
    """A translucent near layer (splat 0, alpha 0.4, depth 3), an opaque far layer (splat 1, depth 6); the occluder goes between."""
    return scene_of([layer(cam, 3.0, 1500.0), layer(cam, 6.0, 1500.0)], [102, 255])


def matrix16(rot_z=0.0, translate=(0.0, 0.0, 0.0), scale=1.0):
    """Column-major 16-vector: rotation about z, uniform scale, translation."""
    c, s_ = np.cos(rot_z), np.sin(rot_z)
    m = np.eye(4)
    m[:3, :3] = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]]) * scale
    m[:3, 3] = translate
    return np.ascontiguousarray(m.T).reshape(16)


def two_scenes(cam):
    """GS_CAM_DYNAMIC: splat 0 belongs to scene 0 (moved left and away), splat 1 to scene 1 (rotated, scaled, moved right and
    nearer) - two opaque 12-px splats that land left and right of the screen centre at different depths.
    Returns (scene, scene indexes, transforms)."""
    transforms = [matrix16(0.0, (-0.45, 0.1, -1.0)), matrix16(0.7, (0.5, -0.1, 1.5), 1.25)]
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    local = (cam.position + (-mw[8:11]) * 4.0).astype(np.float32)
    s = (12.0 * 4.0 / (np.sqrt(8.0) * cam.focal()[1])) ** 2
    parts = [(local[None, :], np.array([[s, 0, 0, s, 0, s]], np.float32))] * 2
    return scene_of(parts, [255, 255]), np.array([0, 1], dtype=np.uint32), transforms


def back_to_front(scene, cam):
    """The draw order of a sorted frame: farthest first (ties by index)."""
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    d = (scene.centers.astype(np.float64) - cam.position) @ (-mw[8:11])
    return np.argsort(-d, kind="stable").astype(np.uint32)


def random_scene(seed):
    return helpers.small_scene(3000, 1, seed)


# -- records without a device: the oracle's vertex stage (what the tolerances are measured on) ---------------------------------------
def oracle_records(scene, cam, w, h):
    """uint32 [n, 8] records as k_project forms them, from the CPU oracle's vertex stage, and the visibility flags."""
    import oracle
    c, cov, rgba, sh = helpers.oracle_inputs(scene)
    ocam = oracle.make_camera(cam.model_view(), cam.projection, cam.position, w, h, scene.sh_degree, scene.sh_degree)
    p = oracle.project(ocam, c, cov, rgba, sh)
    n1 = p["b1x"] * p["b1x"] + p["b1y"] * p["b1y"]
    n2 = p["b2x"] * p["b2x"] + p["b2y"] * p["b2y"]
    k = np.float32(K_POWER)
    with np.errstate(all="ignore"):
        f = np.stack([p["cx"], p["cy"], k * (p["b1x"] / n1), k * (p["b1y"] / n1), k * (p["b2x"] / n2), k * (p["b2y"] / n2)], axis=1).astype(np.float32)
    recs = np.zeros((f.shape[0], 8), dtype=np.uint32)
    recs[:, :6] = f.view(np.uint32)
    a16 = (np.clip(p["a"], 0.0, 1.0) * np.float32(65535.0) + np.float32(0.5)).astype(np.uint32)
    recs[:, 7] = a16 << 16
    vis = (p["visible"] != 0) & np.isfinite(f).all(axis=1)
    return recs, vis


def measure_scene(recs, vis, w, h):
    """(worst power difference, worst relative alpha error) of the kernel's fp32 restatement against fp64 over every visible record
    and every pixel of the frame, bin by bin (a record is staged relative to the bin that evaluates it)."""
    eta = eps = 0.0
    r = recs[vis]
    cx, cy = r[:, 0].copy().view(np.float32), r[:, 1].copy().view(np.float32)
    for by in range((h + 31) // 32):
        for bx in range((w + 31) // 32):
            ys, xs = np.arange(by * 32, min(h, by * 32 + 32)), np.arange(bx * 32, min(w, bx * 32 + 32))
            py, px = (a.ravel() for a in np.meshgrid(ys, xs, indexing="ij"))
            # (records whose centre is absurdly far from the bin cannot reach it: their rect says so and they are never staged)
            sel = (np.abs(cx - (bx * 32 + 16)) < 1100) & (np.abs(cy - (by * 32 + 16)) < 1100)
            e1, e2 = ref.measure_alpha(r[sel], bx, by, px, py)
            eta, eps = max(eta, e1), max(eps, e2)
    return eta, eps


# -- a drawn mesh -> the model's input -------------------------------------------------------------------------------------------
def draw_of(mesh, scene_centers, tile_rows=None, dest_depth=None, unorm24=False, **dynamic):
    """surface_ref.Draw of the mesh's last draw (debug reads, fetched the way tests/test_gpu_bin_lists.py fetches them)."""
    cam = mesh._cam
    list_px = int(mesh.last_stats().list_bin_px)
    ranges, entries, slots = mesh.bin_lists(tile_rows, list_bin_px=list_px)
    recs, rects, vis = mesh.debug_records()
    rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
    r0 = 0 if tile_rows is None else tile_rows[0]
    z = ref.window_depth(scene_centers, list(cam.view), list(cam.proj), **dynamic)
    return ref.Draw(width=int(cam.width), height=int(cam.height), list_shift=(list_px // L.GS_TILE).bit_length() - 1,
                    lists_x=(cam.width + list_px - 1) // list_px, list_row_begin=(r0 * L.GS_TILE) // list_px, ranges=ranges,
                    entries=entries, slots=slots, recs=recs, rects=rects, vis=vis, z=z, dest_depth=dest_depth, unorm24=unorm24)


def entry_index(draw, px, py, splat):
    """Position of `splat` in the list of pixel (px, py)'s list bin (near -> far, 0-based)."""
    per = draw.list_shift - 1
    lid = (((py // 32) >> per) - draw.list_row_begin) * draw.lists_x + ((px // 32) >> per)
    b, e = (int(v) for v in draw.ranges[lid])
    return int(np.nonzero(draw.entries[b:e] == draw.slots[splat])[0][0])
