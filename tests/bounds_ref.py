"""Host model of gs_mesh_bounds (csrc/bounds.hip): numpy fp64, one rounded operation per product / sum / division, in the order
three.js writes them - Vector3.applyMatrix4, Vector3.sub, Vector3.length without the root (SplatMesh.updateVisibleRegion,
src/splatmesh/SplatMesh.js:1172-1199) and the Float32Array store of SplatMesh.computeBoundingBox (:2066-2095)."""
import numpy as np


def apply_matrix4(c64, e):
    """THREE.Vector3.applyMatrix4 of every row of c64 [n, 3] (fp64); e: 16 column-major elements."""
    e = np.asarray(e, np.float64).reshape(16)
    x, y, z = c64[:, 0], c64[:, 1], c64[:, 2]
    with np.errstate(all="ignore"):
        w = 1.0 / (((e[3] * x + e[7] * y) + e[11] * z) + e[15])
        return np.stack([(((e[0] * x + e[4] * y) + e[8] * z) + e[12]) * w,
                         (((e[1] * x + e[5] * y) + e[9] * z) + e[13]) * w,
                         (((e[2] * x + e[6] * y) + e[10] * z) + e[14]) * w], axis=1)


def transformed(centers, transforms=None, scene_idx=None):
    """The fp64 centres the distance sees: the stored fp32 centres widened, or transforms[scene] applied to them."""
    c = np.asarray(centers, np.float32).reshape(-1, 3).astype(np.float64)
    if transforms is None:
        return c
    t = np.asarray(transforms, np.float64).reshape(-1, 16)
    s = np.zeros(c.shape[0], np.int64) if scene_idx is None else np.asarray(scene_idx, np.int64).copy()
    s[s >= t.shape[0]] = 0
    out = np.empty_like(c)
    for k in range(t.shape[0]):
        sel = s == k
        out[sel] = apply_matrix4(c[sel], t[k])
    return out


def bounds(centers, center, start=0, count=None, transforms=None, scene_idx=None):
    """{count, min float32 [3], max float32 [3], max_dist_sq float64} of splats [start, start + count)."""
    c = np.asarray(centers, np.float32).reshape(-1, 3)
    count = c.shape[0] - start if count is None else count
    sl = slice(start, start + count)
    c64 = transformed(c[sl], transforms, None if scene_idx is None else np.asarray(scene_idx)[sl])
    box = c[sl] if transforms is None else c64.astype(np.float32)
    ok = ~np.isnan(c64).any(axis=1)                           # a NaN component: the splat takes part in nothing
    n = int(ok.sum())
    if n == 0:
        return {"count": 0, "min": np.zeros(3, np.float32), "max": np.zeros(3, np.float32), "max_dist_sq": 0.0}
    with np.errstate(all="ignore"):
        d = c64[ok] - np.asarray(center, np.float64).reshape(1, 3)
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    m = 0.0
    for v in s.tolist():                                      # `d > m` from 0, as the reference's running maximum
        if v > m:
            m = v
    return {"count": n, "min": box[ok].min(axis=0), "max": box[ok].max(axis=0), "max_dist_sq": float(m)}
