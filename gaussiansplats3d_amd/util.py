"""Host-side numeric helpers that mirror what the reference's JS layer does before data reaches the GPU."""
import math

import numpy as np


def to_half_three(values):
    """THREE.DataUtils.toHalfFloat (three r160; used by /root/reference/src/loaders/SplatBuffer.js:9,469-474):
    clamp to +-65504, then TRUNCATE the fp32 mantissa via the base/shift tables (no rounding).
    Returns uint16 half bit patterns."""
    v = np.clip(np.asarray(values, dtype=np.float32), -65504.0, 65504.0)
    f = v.view(np.uint32)
    sign = (f >> 16) & 0x8000
    e = ((f >> 23) & 0xFF).astype(np.int32) - 127
    m = f & 0x007FFFFF
    out = np.zeros(f.shape, dtype=np.uint32)
    # e < -24 -> signed zero ; -24 <= e < -14 -> subnormal ; -14 <= e <= 15 -> normal ; e == 128 -> inf/nan
    sub = (e >= -24) & (e < -14)
    sh = np.where(sub, -e - 1, 13).astype(np.uint32)
    out = np.where(sub, (0x0400 >> np.clip(-e - 14, 0, 31).astype(np.uint32)) + (m >> sh), out)
    nor = (e >= -14) & (e <= 15)
    out = np.where(nor, (((e + 15).astype(np.uint32)) << 10) + (m >> 13), out)
    big = (e > 15) & (e < 128)
    out = np.where(big, 0x7C00, out)
    nan = e == 128
    out = np.where(nan, 0x7C00 + (m >> 13), out)
    return (out | sign).astype(np.uint16)


def integer_centers(centers3):
    """SplatMesh.getIntegerCenters(padFour=true), /root/reference/src/splatmesh/SplatMesh.js:1912-1926:
    Math.round(fp32 * 1000.0) in fp64 (round half up), w = 1000."""
    c = np.ascontiguousarray(centers3, dtype=np.float32).reshape(-1, 3)
    out = np.empty((c.shape[0], 4), dtype=np.int32)
    out[:, :3] = np.floor(c.astype(np.float64) * 1000.0 + 0.5).astype(np.int32)
    out[:, 3] = 1000
    return out


def float_centers(centers3):
    """SplatMesh.getFloatCenters(padFour=true), SplatMesh.js:1935-1948: w = 1.0."""
    c = np.ascontiguousarray(centers3, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([c, np.ones((c.shape[0], 1), np.float32)], axis=1)


# -- gpuAcceleratedSort: the uniforms of the distance pass (SplatMesh.computeDistancesOnGPU, SplatMesh.js:1701-1814) ------------
def js_math_round(x):
    """JS Math.round of an fp64 value: the nearest integer, halves towards +Infinity (Python's round() sends halves to even).
    Returned as a float, like the JS number (NaN and infinities pass through)."""
    x = float(x)
    if x != x or x in (math.inf, -math.inf):
        return x
    r = math.floor(x)
    return float(r + 1) if x - r >= 0.5 else float(r)


def js_to_int32(x):
    """ECMAScript ToInt32 / WebIDL `long` (what gl.uniform*i and an Int32Array store make of a JS number): NaN and infinities
    -> 0, otherwise the integer part modulo 2^32 as a signed value."""
    x = float(x)
    if x != x or x in (math.inf, -math.inf):
        return 0
    v = int(x) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def get_integer_matrix_array(elements):
    """SplatMesh.getIntegerMatrixArray (SplatMesh.js:2057-2064): Math.round(m * 1000.0) per element, fp64 (JS numbers)."""
    return [js_math_round(float(e) * 1000.0) for e in np.asarray(elements, dtype=np.float64).reshape(16)]


def premultiply(a, b):
    """THREE.Matrix4: b.clone().premultiply(a) = multiplyMatrices(a, b), fp64, each element summed left to right as three does
    (numpy's matmul may reorder or fuse).  a, b, result: column-major 16-vectors."""
    a = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(16)]
    b = [float(v) for v in np.asarray(b, dtype=np.float64).reshape(16)]
    out = [0.0] * 16
    for col in range(4):
        for row in range(4):
            out[4 * col + row] = a[row] * b[4 * col] + a[4 + row] * b[4 * col + 1] + a[8 + row] * b[4 * col + 2] + a[12 + row] * b[4 * col + 3]
    return out


def distance_uniforms(model_view_proj, integer, dynamic, scene_transforms=None):
    """What computeDistancesOnGPU uploads (SplatMesh.js:1719-1743), in the layout gs_mesh_compute_distances takes:
    static integer int32[3], static float float32[3], dynamic integer int32[4 * scenes], dynamic float float32[16 * scenes]
    (per scene mvp * transform).  Returns (array, scene_count)."""
    mvp = [float(v) for v in np.asarray(model_view_proj, dtype=np.float64).reshape(16)]
    if not dynamic:
        if integer:
            im = get_integer_matrix_array(mvp)
            return np.array([js_to_int32(im[k]) for k in (2, 6, 10)], dtype=np.int32), 1
        return np.array([mvp[2], mvp[6], mvp[10]], dtype=np.float64).astype(np.float32), 1
    transforms = [np.eye(4).reshape(16)] if scene_transforms is None or len(scene_transforms) == 0 else scene_transforms
    rows = []
    for t in transforms:
        m = premultiply(mvp, t)
        if integer:
            im = get_integer_matrix_array(m)
            rows += [js_to_int32(im[k]) for k in (2, 6, 10, 14)]
        else:
            rows += m
    out = np.array(rows, dtype=np.int32) if integer else np.array(rows, dtype=np.float64).astype(np.float32)
    return out, len(transforms)


def remove_args(ranges, scene_remap):
    """The arguments of gs_mesh_remove / gs_sorter_remove: (ranges uint32 [n, 2] of (from, count) pairs, n, scene_remap uint32
    array or None, its length)."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if r.size and (r.min() < 0 or r.max() > 0xFFFFFFFF):
        raise ValueError("ranges must hold unsigned 32-bit (from, count) pairs")
    r = np.ascontiguousarray(r.astype(np.uint32))
    m = None if scene_remap is None else np.ascontiguousarray(scene_remap, dtype=np.uint32).reshape(-1)
    return r, r.shape[0], m, 0 if m is None else m.size


def removed_below(ranges, count):
    """How many of the positions [0, count) the (from, count) ranges of an accepted removal take away."""
    return sum(max(0, min(start + n, count) - min(start, count)) for start, n in np.asarray(ranges, dtype=np.int64).reshape(-1, 2).tolist())
