"""numpy restatement of the gpuAcceleratedSort distance pass (SplatMesh.computeDistancesOnGPU, SplatMesh.js:1701-1814, and the
transform-feedback shader of :1449-1490): the checker of tests/test_distances_uniforms.py and tests/test_gpu_distances.py."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def js_integer_centers(centers3):
    """getIntegerCenters(padFour) as an Int32Array stores it: ToInt32(Math.round(fp32 * 1000.0)) - NaN / infinities -> 0, the
    rest wrapped modulo 2^32 - and w = 1000.  int32[n, 4]."""
    t = np.asarray(centers3, dtype=np.float32).reshape(-1, 3).astype(np.float64) * 1000.0
    t = np.where(np.isfinite(t), t, 0.0)
    r = np.floor(t)
    r = r + (t - r >= 0.5)                                   # Math.round: halves towards +Infinity, exact for any |t|
    m = r - 4294967296.0 * np.floor(r / 4294967296.0)        # exact: an integer in [0, 2^32)
    out = np.empty((t.shape[0], 4), dtype=np.int32)
    out[:, :3] = m.astype(np.uint64).astype(np.uint32).view(np.int32)
    out[:, 3] = 1000
    return out


def shader_distances(centers4, uniforms, integer, dynamic, scene_indexes=None):
    """The four permutations of the distance shader over padFour centres (int32[n,4] or float32[n,4]).  uniforms in the layout of
    gs_mesh_compute_distances.  integer: GLSL int arithmetic wraps (done in uint32); float: fp32, unfused, left to right."""
    c = np.asarray(centers4)
    n = c.shape[0]
    sc = np.zeros(n, np.int64) if scene_indexes is None else np.asarray(scene_indexes, np.int64) & 31
    with np.errstate(over="ignore", invalid="ignore"):
        if integer:
            x, y, z, w = (c[:, k].astype(np.int32).view(np.uint32) for k in range(4))
            u = np.asarray(uniforms, dtype=np.int32).view(np.uint32)
            if dynamic:
                rows = np.zeros((32, 4), np.uint32)
                rows[:u.size // 4] = u.reshape(-1, 4)
                r = rows[sc]
                d = x * r[:, 0] + y * r[:, 1] + z * r[:, 2] + r[:, 3] * w
            else:
                d = x * u[0] + y * u[1] + z * u[2]
            return d.astype(np.uint32).view(np.int32)
        x, y, z = (c[:, k].astype(np.float32) for k in range(3))
        u = np.asarray(uniforms, dtype=np.float32)
        if dynamic:
            rows = np.zeros((32, 4), np.float32)
            rows[:u.size // 16] = u.reshape(-1, 16)[:, [2, 6, 10, 14]]
            r = rows[sc]
            s = r[:, 0] * x
            s = s + r[:, 1] * y
            s = s + r[:, 2] * z
            return (s + r[:, 3]).astype(np.float32)
        s = x * u[0]
        s = s + y * u[1]
        return (s + z * u[2]).astype(np.float32)


def shim_centers(centers3):
    """(int32[n,4], float32[n,4]): what node/SplatMesh.mjs's own getIntegerCenters / getFloatCenters (padFour) make of these fp32
    centres (tests/shim_centers.mjs under Node).  None when Node is not installed."""
    if shutil.which("node") is None:
        return None
    c = np.ascontiguousarray(centers3, dtype=np.float32).reshape(-1, 3)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "node")], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as d:
        src, ip, fp = (os.path.join(d, f) for f in ("in.f32", "out.i32", "out.f32"))
        c.tofile(src)
        subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                               os.path.join(ROOT, "tests", "shim_centers.mjs"), src, ip, fp], cwd=os.path.join(ROOT, "tests"),
                              stdout=subprocess.DEVNULL, timeout=600)
        return np.fromfile(ip, dtype=np.int32).reshape(-1, 4), np.fromfile(fp, dtype=np.float32).reshape(-1, 4)
