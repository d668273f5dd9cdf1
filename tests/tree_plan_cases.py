"""Scenes with exact leaf control and camera scripts for the octree gather's plan (csrc/tree.hip: k_tree_test, k_tree_scan,
k_tree_fill, k_tree_offsets), shared by tests/test_tree_plan_ref.py (host model) and tests/test_gpu_tree_plan.py (device).

LATTICE scenes: the box [-4, 4]^3 cut into G^3 cells, max_depth = log2(G) - 1, max_centers = 2.  K chosen cells hold 2 to 5
centres each, strictly inside (0.2 to 0.8 of the cell); cells (0,0,0) and (G-1,G-1,G-1) are always chosen and hold one more centre
on the box's min / max corner, which pins the scene box.  Every node above depth log2(G) then holds >= 2 centres and splits, every
chosen cell is a leaf at depth log2(G) whose centre is the cell's centre (dyadic: exact), so the tree has exactly K leaves with
different splat counts.  The upload order is permuted.

A SCRIPT is a list of steps played in order on ONE tree: the plan's tables (fill, hist, the previous keys, prev_scale) are carried
from gather to gather, so the order is the subject.  Eye distances are in scene half-sizes.

The module also restates the host's bucket scale (gs_tree_gather: farthest of the 8 box corners, * 1.0001) and tree_bucket, from
which `step_report` counts, per step: leaves kept, occupancy per bucket, exact ties and near ties.
"""
import functools
import math
import struct

import numpy as np

TREE_BUCKET_BITS = 18
TREE_BUCKETS = 1 << TREE_BUCKET_BITS

# name -> (G, K); the L = 1 tree is a single splat, `clusters10k` is ordinary one-leaf-per-bucket content
LATTICES = {"lat1": (0, 1), "lat2": (8, 2), "lat8": (8, 8), "lat9": (8, 9), "lat16": (8, 16), "lat17": (8, 17), "lat255": (8, 255),
            "lat256": (8, 256), "lat257": (8, 257), "lat512": (8, 512), "lat1025": (16, 1025)}
SCENES = list(LATTICES) + ["clusters10k"]
SINGLE_SPLAT = (0.5, -1.25, 2.0)


def _seed(name):
    return sum(ord(ch) for ch in name) * 7919


@functools.lru_cache(maxsize=None)
def make_scene(name):
    """dict(centers float32 [n,3], max_depth, max_centers, leaves_expected or None)"""
    rng = np.random.default_rng(_seed(name))
    if name == "clusters10k":               # tree_cases' clusters40k, cut to 10 k centres
        k = rng.uniform(-4, 4, size=(40, 3))
        c = (k[rng.integers(0, 40, 10000)] + rng.normal(size=(10000, 3)) * 0.2).astype(np.float32)
        return dict(centers=c, max_depth=8, max_centers=100, leaves_expected=None)
    G, K = LATTICES[name]
    if K == 1:
        return dict(centers=np.array([SINGLE_SPLAT], np.float32), max_depth=8, max_centers=2, leaves_expected=1)
    cell = 8.0 / G
    corners = [0, G ** 3 - 1]                                  # flat index of (0,0,0) and (G-1,G-1,G-1)
    rest = np.setdiff1d(np.arange(G ** 3), corners)
    chosen = np.concatenate([corners, rng.permutation(rest)[:K - 2]])
    pts = []
    for flat in chosen:
        ijk = np.array([flat // (G * G), (flat // G) % G, flat % G], np.float64)
        m = int(rng.integers(2, 6))
        pts.append(-4.0 + (ijk[None, :] + rng.uniform(0.2, 0.8, size=(m, 3))) * cell)
    pts.append(np.array([[-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]]))
    c = np.concatenate(pts).astype(np.float32)
    c = c[rng.permutation(len(c))]
    assert len(c) < 6000
    return dict(centers=c, max_depth=int(math.log2(G)) - 1, max_centers=2, leaves_expected=K)


@functools.lru_cache(maxsize=None)
def oracle_leaves(name):
    """oracle/tree_oracle.py::build_tree of the scene (computed once, shared; callers must not change it)"""
    from oracle import tree_oracle
    s = make_scene(name)
    leaves, _ = tree_oracle.build_tree(s["centers"], None, s["max_depth"], s["max_centers"])
    return leaves


def _diag(lf):
    """nodeSize: the leaf box's diagonal"""
    dx, dy, dz = (lf["max"][k] - lf["min"][k] for k in range(3))
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def scene_box(centers):
    """(min, max) of the uploaded fp32 centres, as doubles: gs_tree_create's scene box"""
    c = np.asarray(centers, np.float32).reshape(-1, 3).astype(np.float64)
    return c.min(axis=0), c.max(axis=0)


# ------------------------------------------------------------------------------------------------ cameras
def _rigid(rot, eye):
    """column-major modelView of v = rot @ (x - eye)"""
    m = np.eye(4)
    m[:3, :3] = rot
    m[:3, 3] = -(np.asarray(rot, np.float64) @ np.asarray(eye, np.float64))
    return np.ascontiguousarray(m.T).reshape(16)


def _look(eye, target, up=(0.0, 1.0, 0.0)):
    """three.js lookAt: the camera looks down -Z at the target"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = eye - target
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return _rigid(np.stack([x, y, z]), eye)


def _step(tag, mv, fov=50.0, width=1280, height=720, gather_all=False):
    return dict(tag=tag, model_view=np.asarray(mv, np.float64).reshape(16), fov=float(fov), width=int(width), height=int(height),
                gather_all=bool(gather_all))


@functools.lru_cache(maxsize=None)
def make_script(name):
    """The steps of the scene's script, in playing order (the tags name the rows of the issue's table)."""
    leaves = oracle_leaves(name)
    mn, mx = scene_box(make_scene(name)["centers"])
    mid = (mn + mx) * 0.5
    half = float(np.max(mx - mn)) * 0.5 or 1.0              # the single splat's box is a point
    d1 = np.array([0.48, 0.64, 0.6])                        # unit directions the far eyes sit on
    d2 = np.array([-0.6, 0.0, 0.8])
    inside = mid + half * np.array([0.075, -0.175, 0.275])
    off_centre = mid + half * np.array([0.75, 0.5, -0.25])
    pose_a = _look(inside, off_centre)
    far_eye = lambda k, d: _look(mid + d * (k * half), mid)     # noqa: E731
    on_leaf = np.array(leaves[len(leaves) // 2]["center"], np.float64)
    # an integer eye outside the lattice, looking at the origin: the rotation's entries are irrational, so leaves that would tie
    # exactly under an exact rotation round apart by a few ulp (and some still tie)
    pose_f = _look((9.0, 3.0, 5.0), (0.0, 0.0, 0.0))
    behind = _rigid(np.eye(3), mid + np.array([0.0, 0.0, -25.0 * half]))      # looks down -Z from below the scene: all of it behind
    non_affine = _rigid(np.eye(3), (0.0, 0.0, 10.0))                          # translation (0, 0, -10) ...
    non_affine[11] = -100.0                                                   # ... and a w row three.js never produces
    steps = [
        _step("a", pose_a),
        _step("b", far_eye(1e3, d1)),
        _step("c", far_eye(1e5, d1)),
        _step("d", far_eye(1e7, d1)),
        _step("e", pose_a),
        _step("d2", far_eye(1e7, d1)),                       # straight from the inside pose: the scale falls by > 1e6
        _step("f", pose_f),
        _step("g", _rigid(np.eye(3), (0.0, 0.0, 0.0)), gather_all=True),   # every leaf: the lattice's symmetric partners tie exactly
        _step("h", _rigid(np.eye(3), on_leaf)),
        _step("i", behind),
        _step("j", behind, gather_all=True),
        _step("a2", pose_a),
        _step("k", pose_a, fov=25.0, width=500, height=900),
        _step("l", non_affine),
        _step("c2", far_eye(1e5, d2)),
        _step("a3", pose_a),
    ]
    if name == "lat1":                                       # eye ON the only splat: far == 0, scale = 1.0
        assert np.array_equal(on_leaf, np.array(SINGLE_SPLAT, np.float32).astype(np.float64))
    return steps


@functools.lru_cache(maxsize=None)
def oracle_lists(name):
    """oracle/tree_oracle.py::gather at every step of the scene's script (computed once, shared; callers must not change them)"""
    from oracle import tree_oracle
    leaves = oracle_leaves(name)
    out = []
    for s in make_script(name):
        lst = tree_oracle.gather(leaves, s["model_view"], s["fov"], s["width"], s["height"], s["gather_all"])
        lst.setflags(write=False)
        out.append(lst)
    return out


def sort_mvp(step):
    """A modelViewProj for the sorts that consume the step's list: three.js perspective (near 0.1, far 1000) * modelView."""
    from gaussiansplats3d_amd import camera
    return camera.multiply(camera.make_perspective(step["fov"], step["width"] / step["height"], 0.1, 1000.0), step["model_view"])


# ------------------------------------------------------------------------------------------------ host restatements
def host_scale(scene_min, scene_max, model_view):
    """gs_tree_gather's bucket scale: TREE_BUCKETS / (far * 1.0001), far = the farthest of the 8 scene-box corners."""
    e = [float(v) for v in np.asarray(model_view, np.float64).reshape(16)]
    far = 0.0
    for c in range(8):
        x = float(scene_max[0] if c & 1 else scene_min[0])
        y = float(scene_max[1] if c & 2 else scene_min[1])
        z = float(scene_max[2] if c & 4 else scene_min[2])
        w = e[3] * x + e[7] * y + e[11] * z + e[15]
        w = 1.0 / w if w != 0.0 else 1.0
        vx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w
        vy = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w
        vz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w
        d = math.sqrt(vx * vx + vy * vy + vz * vz)
        if d > far:
            far = d
    return float(TREE_BUCKETS) / (far * 1.0001) if 0.0 < far < 1e300 else 1.0


def tree_bucket(key, scale):
    """tree.hip's tree_bucket for a finite key >= 0"""
    b = key * scale
    return int(b) if b < float(TREE_BUCKETS - 1) else TREE_BUCKETS - 1


def leaf_keys(leaves, step):
    """Per leaf: the fp64 distance of Viewer.gatherSceneNodesForSort, None when the leaf is culled (plain Python doubles, the
    operation order of oracle/tree_oracle.py::gather)."""
    e = [float(v) for v in step["model_view"]]
    focal = (step["height"] / 2.0) / math.tan(step["fov"] / 2.0 * (math.pi / 180.0))
    cos_x = math.cos(math.atan(step["width"] / 2.0 / focal))
    cos_y = math.cos(math.atan(step["height"] / 2.0 / focal))
    keys = []
    for lf in leaves:
        x, y, z = lf["center"]
        w = 1.0 / (e[3] * x + e[7] * y + e[11] * z + e[15])
        vx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w
        vy = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w
        vz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w
        dist = math.sqrt(vx * vx + vy * vy + vz * vz)
        s = 1.0 / (dist or 1.0)
        vx, vy, vz = vx * s, vy * s, vz * s
        lyz = math.sqrt(0.0 * 0.0 + vy * vy + vz * vz)
        yz_z = vz * (1.0 / (lyz or 1.0))
        lxz = math.sqrt(vx * vx + 0.0 * 0.0 + vz * vz)
        xz_z = vz * (1.0 / (lxz or 1.0))
        out = -yz_z < (cos_y - .6) or -xz_z < (cos_x - .6)
        keys.append(None if (not step["gather_all"] and out and dist > _diag(lf)) else dist)
    return keys


def _bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


@functools.lru_cache(maxsize=None)
def step_report(name, k):
    """What step k of the scene's script gives the plan: dict(leaves, kept, scale, occupancy {bucket: leaf count}, members {bucket:
    [leaf]}, max_occupancy, ties, near_ties, clamp).  ties = kept leaves minus distinct keys; near_ties = pairs of kept leaves whose
    keys differ by 1 to 4 ulp; clamp = leaves in bucket 2^18 - 1.  (Computed once, shared; callers must not change it.)"""
    leaves = oracle_leaves(name)
    step = make_script(name)[k]
    mn, mx = scene_box(make_scene(name)["centers"])
    scale = host_scale(mn, mx, step["model_view"])
    kept = [(i, d) for i, d in enumerate(leaf_keys(leaves, step)) if d is not None]
    occ = {}
    for i, d in kept:
        occ.setdefault(tree_bucket(d, scale), []).append(i)
    bits = np.sort(np.array([_bits(d) for _, d in kept], np.int64))
    vals, cnt = np.unique(bits, return_counts=True)
    near = 0
    for u in range(1, 5):                                    # pairs of DISTINCT key values u ulp apart, times their multiplicities
        pos = np.searchsorted(vals, vals + u)
        hit = (pos < len(vals)) & (vals[np.minimum(pos, len(vals) - 1)] == vals + u)
        near += int((cnt[hit] * cnt[pos[hit]]).sum())
    return dict(leaves=len(leaves), kept=len(kept), scale=scale, occupancy={b: len(v) for b, v in occ.items()}, members=occ,
                max_occupancy=max((len(v) for v in occ.values()), default=0), ties=len(bits) - len(vals), near_ties=near,
                clamp=len(occ.get(TREE_BUCKETS - 1, [])))
