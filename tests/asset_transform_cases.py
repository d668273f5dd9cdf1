"""What tests/test_assets_transform_ref.py (CPU) and tests/test_gpu_asset_transform.py (-m gpu) share: the goldens recorded by
tests/tools/make_assets_transform_golden.py, the five transforms, and the per-case cameras with the numpy frustum test that
holds them to "at least a quarter of the splats in view"."""
import json
import os

import numpy as np

from gaussiansplats3d_amd import camera

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["sh2", "sh1", "sh0"]
TAGS = ["ply", "gen0", "gen1", "gen2"]
TRANSFORMS = ["identity", "rigid", "uniform", "nonuniform", "mirror"]
CLUSTER = (2.4, 2.6, -2.5)            # 62 % of a golden file's splats, sigma 0.25 (oracle/make_golden_assets.py)
W, H = 320, 180
MIN_IN_VIEW = 0.25

_CACHE = {}


def golden(case):
    """(inputs npz, their manifest, transformed npz, its manifest), loaded once."""
    if case not in _CACHE:
        g = np.load(os.path.join(GOLDEN, f"assets_ref_{case}.npz"))
        t = np.load(os.path.join(GOLDEN, f"assets_transform_ref_{case}.npz"))
        _CACHE[case] = ({k: g[k] for k in g.files}, json.loads(bytes(g["manifest"]).decode()),
                        {k: t[k] for k in t.files}, json.loads(bytes(t["manifest"]).decode()))
    return _CACHE[case]


def file_of(case, tag):
    g, man, _, _ = golden(case)
    if tag == "ply":
        return bytes(g["ply_bytes"]), "ply", man["shDegree"]
    return bytes(g[f"{tag}_ksplat"]), "ksplat", man["shDegree"]


def matrix(name):
    return golden("sh0")[2][f"{name}_matrix"].copy()


def apply(m16, p):
    m = np.asarray(m16, np.float64).reshape(4, 4).T
    return m[:3, :3] @ np.asarray(p, np.float64) + m[:3, 3]


def scene_scale(m16):
    m = np.asarray(m16, np.float64).reshape(4, 4).T
    return abs(np.linalg.det(m[:3, :3])) ** (1.0 / 3.0)


def camera_at(target, distance):
    """Looks at `target` from `distance` away along a fixed oblique direction."""
    d = np.array([0.35, 0.25, 1.0])
    d /= np.linalg.norm(d)
    return camera.PerspectiveCamera(W, H, tuple(np.asarray(target) + distance * d), tuple(target), (0.0, 1.0, 0.0))


def golden_camera(name):
    """The camera of a golden case under transform `name`: at the transformed cluster centre from six scene-scaled units."""
    m = matrix(name)
    return camera_at(apply(m, CLUSTER), 6.0 * scene_scale(m))


def cloud_camera(centers):
    """For any other file: at the median of its finite centres from 2.5 times their median distance to it."""
    c = np.asarray(centers, np.float64)
    c = c[np.isfinite(c).all(axis=1)]
    mid = np.median(c, axis=0)
    return camera_at(mid, 2.5 * np.median(np.linalg.norm(c - mid, axis=1)))


def share_in_view(centers, cam):
    """Share of the centres strictly inside the camera's frustum (clip-space test on proj * view * centre)."""
    c = np.asarray(centers, np.float64)
    mvp = np.asarray(cam.sort_mvp(), np.float64).reshape(4, 4).T
    with np.errstate(all="ignore"):
        clip = np.concatenate([c, np.ones((len(c), 1))], axis=1) @ mvp.T
        w = clip[:, 3:4]
        inside = (w[:, 0] > 0) & (np.abs(clip[:, :3]) < w).all(axis=1)
    return float(inside.mean())
