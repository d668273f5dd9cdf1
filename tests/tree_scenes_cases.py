"""Dynamic-mode meshes for the per-scene octree cull (csrc/tree.hip: gs_tree_create_scenes, gs_tree_gather_scenes,
k_tree_test_scenes), shared by tests/tools/make_tree_scenes_golden.py (records the reference), tests/test_tree_scenes_ref.py (host
model) and tests/test_gpu_tree_scenes.py (device).

A SCENE is a lattice in the manner of tests/tree_plan_cases.py: the box [-4, 4]^3 cut into 8^3 cells, max_depth 2, max_centers 2,
K chosen cells of 2 to 5 centres each plus the two box corners, which gives exactly K leaves with different splat counts; K = 1 is a
single splat.  The `dropin` case has two cluster scenes of 3000 splats at the tree parameters SplatMesh.buildSplatTree fixes (depth 8,
1000 centres per node), for the drop-in mesh of tests/test_node_tree_scenes.py.  A CASE is a list of scenes, one transform per scene,
a mesh matrixWorld (which dynamic mode must NOT use), an optional alpha filter and a camera script of a few poses played in order on
ONE tree.
"""
import functools

import numpy as np

MAX_SCENES = 32
MAX_DEPTH, MAX_CENTERS = 2, 2
G = 8


def _seed(name):
    return sum(ord(ch) for ch in name) * 7919


def lattice(rng, K):
    """float32 [n,3]: a scene of exactly K leaves"""
    if K == 1:
        return rng.uniform(-3.0, 3.0, size=(1, 3)).astype(np.float32)
    cell = 8.0 / G
    corners = [0, G ** 3 - 1]
    rest = np.setdiff1d(np.arange(G ** 3), corners)
    chosen = np.concatenate([corners, rng.permutation(rest)[:K - 2]])
    pts = []
    for flat in chosen:
        ijk = np.array([flat // (G * G), (flat // G) % G, flat % G], np.float64)
        m = int(rng.integers(2, 6))
        pts.append(-4.0 + (ijk[None, :] + rng.uniform(0.2, 0.8, size=(m, 3))) * cell)
    pts.append(np.array([[-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]]))
    c = np.concatenate(pts).astype(np.float32)
    return c[rng.permutation(len(c))]


# ------------------------------------------------------------------------------------------------ transforms (column-major)
def _elements(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T).reshape(16)


IDENTITY = _elements(np.eye(4))


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return _elements(m)


def rot_translation(axis, angle, x, y, z):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)
    m[:3, 3] = (x, y, z)
    return _elements(m)


def scale_translation(sx, sy, sz, x, y, z):
    m = np.diag([sx, sy, sz, 1.0])
    m[:3, 3] = (x, y, z)
    return _elements(m)


MESH_WORLD = rot_translation((0.3, 1.0, -0.2), 0.45, 0.75, -1.25, 2.5)      # dynamic mode leaves it out of the base (Viewer.js:2000)

# name -> (leaves per scene, transform per scene); alpha filters below
_R1 = rot_translation((0.0, 1.0, 0.0), 0.7, 9.0, -0.5, 0.25)
_R2 = rot_translation((1.0, 0.4, -0.3), -1.1, -3.0, 6.0, -7.5)
_T1 = translation(-10.0, 2.0, 1.5)
_S1 = scale_translation(0.5, 2.0, 1.25, 2.0, -9.0, 4.0)
_KINDS = (IDENTITY, _T1, _R1, _S1, _R2)
CASES = {
    "two": ((40, 57), (IDENTITY, _R1)),
    "three": ((30, 1, 300), (_T1, _S1, _R2)),
    "max": (tuple(2 + (s * 7) % 5 for s in range(MAX_SCENES)),
            tuple(_KINDS[s % 5] if s < 5 else rot_translation((1.0, s, -2.0), 0.1 * s, 3.0 * (s % 7) - 9.0, 2.0 * (s % 5) - 4.0, 1.5 * s - 20.0)
                  for s in range(MAX_SCENES))),
    "flat255": ((100, 155), (_R2, _T1)),                # a scene boundary inside the test kernel's only workgroup
    "flat256": ((128, 128), (_S1, IDENTITY)),           # the leaf table fills the workgroup exactly
    "flat257": ((256, 1), (_R1, _T1)),                  # the boundary ON the workgroup's edge: the second workgroup is scene 1 alone
    "twins": ((64, 64), (IDENTITY, IDENTITY)),          # the same points under the same transform: every leaf ties across sub-trees
    "culled_kept": ((20, 24), (translation(0.0, 0.0, 60.0), translation(0.0, 0.0, -14.0))),
    "alpha": ((25, 18, 33), (IDENTITY, _R1, _T1)),      # scene 1's filter keeps nothing, scene 2's about half
    "dropin": ((None, None), (IDENTITY, rot_translation((0.0, 1.0, 0.0), 0.7, 40.0, -0.5, 0.25))),   # the drop-in's own tree parameters
}
DROPIN_SPLATS, DROPIN_DEPTH, DROPIN_CENTERS = 3000, 8, 1000
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(name, seed, centers float32 [n,3] (scenes back to back), scene_counts, scene_leaves (expected, None under a filter),
    transforms float64 [S,16], mesh_world, alphas / min_alphas or None, max_depth, max_centers)"""
    rng = np.random.default_rng(_seed(name))
    ks, transforms = CASES[name]
    if name == "twins":
        one = lattice(rng, ks[0])
        scenes = [one, one.copy()]
    elif name == "dropin":
        scenes = []
        for _ in ks:
            k = rng.uniform(-3.5, 3.5, size=(20, 3))
            scenes.append((k[rng.integers(0, 20, DROPIN_SPLATS)] + rng.normal(size=(DROPIN_SPLATS, 3)) * 0.3).astype(np.float32))
    else:
        scenes = [lattice(rng, k) for k in ks]
    counts = np.array([len(s) for s in scenes], np.uint32)
    alphas = min_alphas = None
    expected = list(ks) if name != "dropin" else None
    if name == "alpha":
        alphas = rng.integers(1, 256, size=int(counts.sum())).astype(np.uint8)
        a, b = int(counts[0]), int(counts[0] + counts[1])
        alphas[a:b] = rng.integers(0, 40, size=b - a)          # all below scene 1's minAlpha
        min_alphas = [1, 40, 128]
        expected = None
    return dict(name=name, seed=_seed(name), centers=np.concatenate(scenes), scene_counts=counts, scene_leaves=expected,
                transforms=np.stack([np.asarray(t, np.float64) for t in transforms]), mesh_world=MESH_WORLD, alphas=alphas,
                min_alphas=min_alphas, max_depth=DROPIN_DEPTH if name == "dropin" else MAX_DEPTH,
                max_centers=DROPIN_CENTERS if name == "dropin" else MAX_CENTERS)


def keep_mask(case):
    """SplatMesh.buildSplatTree's filter, per scene: alpha >= minAlphas[s]"""
    if case["alphas"] is None:
        return None
    return case["alphas"] >= np.repeat(np.asarray(case["min_alphas"]), case["scene_counts"])


def scene_ranges(case):
    first = np.concatenate([[0], np.cumsum(case["scene_counts"].astype(np.int64))])
    return [(int(first[s]), int(first[s + 1])) for s in range(len(case["scene_counts"]))]


# ------------------------------------------------------------------------------------------------ camera scripts
def _pose(tag, position, target, up=(0.0, 1.0, 0.0), fov=50.0, width=1280, height=720, gather_all=False):
    from gaussiansplats3d_amd import camera
    return dict(tag=tag, matrix_world=np.asarray(camera.look_at_world(position, target, up), np.float64).reshape(16), fov=float(fov),
                width=int(width), height=int(height), gather_all=bool(gather_all))


@functools.lru_cache(maxsize=None)
def make_script(name):
    """The case's camera poses, in playing order (camera.matrixWorld; the base modelView is its inverse, recorded in the golden)."""
    if name == "culled_kept":
        # looks down -Z from the origin: scene 0 sits 60 behind the eye (entirely culled), scene 1 14 ahead (entirely kept)
        return [_pose("ahead", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=80.0, width=1000, height=1000),
                _pose("all", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), fov=80.0, width=1000, height=1000, gather_all=True),
                _pose("turned", (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fov=80.0, width=1000, height=1000)]
    poses = [_pose("a", (0.5, 0.3, 6.0), (0.0, 0.0, 0.0)),
             _pose("b", (-30.0, 12.0, 4.0), (9.0, 0.0, 0.0), fov=75.0, width=640, height=480),
             _pose("all", (0.5, 0.3, 6.0), (0.0, 0.0, 0.0), gather_all=True),
             _pose("c", (9.0, 3.0, 5.0), (-10.0, 2.0, 1.5), up=(0.0, 0.0, 1.0), fov=30.0, width=300, height=900),
             _pose("d", (1.0, 0.5, -0.5), (9.0, -0.5, 0.25), fov=40.0, width=800, height=600),      # inside the lattice at the origin
             _pose("a2", (0.5, 0.3, 6.0), (0.0, 0.0, 0.0))]
    if name == "dropin":
        # scene 0 sits at the origin, scene 1 40 away along x, the eye between them.  `toward1` keeps scene 1 alone - and a tree
        # that tests scene 1's leaves under scene 0's transform sees them at the origin, behind the eye, and drops every one
        return [_pose("toward1", (20.0, 0.0, 0.0), (40.0, 0.0, 0.0)), _pose("toward0", (20.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                _pose("side", (20.0, 0.0, 30.0), (20.0, 0.0, 0.0)), _pose("all", (20.0, 0.0, 0.0), (40.0, 0.0, 0.0), gather_all=True)]
    if name == "twins":
        # the eye on the lattice's centre, axis-aligned (modelView = identity, exactly): mirror partners tie exactly, inside each
        # sub-tree and across the two, so leaves with DIFFERENT numbers inside their sub-trees tie across sub-trees
        poses.insert(1, dict(tag="ties", matrix_world=np.asarray(IDENTITY, np.float64), fov=50.0, width=1280, height=720, gather_all=True))
    return poses
