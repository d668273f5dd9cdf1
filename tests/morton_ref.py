"""Host model (numpy, float32) of the storage order of one Morton run (csrc/mesh.hip: mesh_commit_segment's bounds,
k_morton_keys, the stable radix sort): which storage position every splat of a fresh upload - or of a range folded by
gs_mesh_reorder - receives.

Every float operation of the device code is one IEEE float32 operation here, in the same order: per axis a subtraction and two
multiplications, `(v - lo) * inv * 1023`.  No addition follows a multiplication, so the compiler has nothing to contract into an
FMA and the model needs no contraction rule; the extent's reciprocal is one division on the host.  The clamp's comparisons are
false for NaN, and the conversion to an integer gives 0 for NaN (`NaN -> 0` in k_morton_keys)."""
import numpy as np

F = np.float32


def bounds(centers):
    """min / max per axis by the host's `v < mn` / `v > mx` tests from +inf / -inf: NaN never moves a bound, an infinity does"""
    c = np.asarray(centers, F).reshape(-1, 3)
    mn, mx = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for k in range(3):
        v = c[:, k][~np.isnan(c[:, k])]
        if v.size:
            mn[k], mx[k] = v.min(), v.max()
    return mn, mx


def _spread(v):
    """10 bits -> every third bit"""
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def keys(centers, mn=None, mx=None):
    """the 30-bit Morton codes k_morton_keys gives the centres under the bounds (default: their own)"""
    c = np.asarray(centers, F).reshape(-1, 3)
    if mn is None:
        mn, mx = bounds(c)
    out = np.zeros(c.shape[0], np.uint32)
    with np.errstate(all="ignore"):
        for k in range(3):
            inv = F(1.0) / F(mx[k] - mn[k]) if mx[k] > mn[k] else F(0.0)
            t = ((c[:, k] - F(mn[k])).astype(F) * F(inv)).astype(F) * F(1023.0)
            t = t.astype(F)
            q = np.where(t < F(0.0), F(0.0), np.where(t > F(1023.0), F(1023.0), t))
            q = np.where(np.isnan(q), F(0.0), q).astype(np.uint32)       # (truncation: the values are in [0, 1023])
            out |= _spread(q) << np.uint32(k)
    return out


def order(centers):
    """the run's local indexes in storage order: ascending key, equal keys in ORIGINAL index order"""
    return np.argsort(keys(centers), kind="stable").astype(np.uint32)


def positions(centers, start=0):
    """storage position by original index of a run uploaded at `start` (what gs_mesh_debug_read 12 returns for it)"""
    o = order(centers)
    pos = np.empty(o.size, np.uint32)
    pos[o] = start + np.arange(o.size, dtype=np.uint32)
    return pos
