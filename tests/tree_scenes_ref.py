"""Host model of the per-scene octree cull (csrc/tree.hip: gs_tree_create_scenes + gs_tree_gather_scenes), pinned to the recorded
reference (tests/golden/tree_scenes_ref.json) by tests/test_tree_scenes_ref.py:

  build    oracle/tree_oracle.py::build_tree per scene over the scene's own centres, first_index = the scene's first global index;
           the flat leaf table is the sub-trees' nodesWithIndexes one after the other, with one scene id per leaf
  gather   modelView_s = base x transform_s (Matrix4.multiplyMatrices' expression order, plain Python doubles); every leaf is tested
           under its scene's modelView with the arithmetic of oracle/tree_oracle.py::gather; kept leaves are ordered by
           (distance, flat leaf number) and laid out far -> near

`gather` takes a MUTATION name; each one is a way to get the feature wrong, and the CPU test shows a recorded case that catches it.
"""
import functools
import json
import math
import os
import struct

import numpy as np

import tree_scenes_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_scenes_ref.json")
MUTATIONS = ("scene0_matrix", "tie_by_local_leaf", "mesh_world_in_base", "transform_times_base", "local_indexes")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_base(name, k):
    """inverse(camera.matrixWorld) of pose k as the reference computed it: float64 [16]"""
    return np.array([struct.unpack("<d", bytes.fromhex(h))[0] for h in golden()[name]["poses"][k]["base"]], np.float64)


@functools.lru_cache(maxsize=None)
def golden_list(name, k):
    lst = np.array(golden()[name]["poses"][k]["indexes"], np.uint32)
    lst.setflags(write=False)
    return lst


def multiply(a, b):
    """Matrix4.multiplyMatrices(a, b): column-major 16-lists, the reference's expression order"""
    a, b = [float(v) for v in a], [float(v) for v in b]
    te = [0.0] * 16
    for c in range(4):
        for r in range(4):
            te[r + 4 * c] = a[r] * b[4 * c] + a[r + 4] * b[4 * c + 1] + a[r + 8] * b[4 * c + 2] + a[r + 12] * b[4 * c + 3]
    return te


@functools.lru_cache(maxsize=None)
def sub_trees(name):
    """[(leaves of scene s in nodesWithIndexes order)] per scene (computed once, shared; callers must not change it)"""
    from oracle import tree_oracle
    case = cases.make_case(name)
    keep = cases.keep_mask(case)
    out = []
    for a, b in cases.scene_ranges(case):
        leaves, _ = tree_oracle.build_tree(case["centers"][a:b], None if keep is None else keep[a:b], case["max_depth"],
                                           case["max_centers"], first_index=a)
        out.append(leaves)
    return out


def leaf_key(leaf, e, cos_x, cos_y, gather_all):
    """Viewer.js:2016-2032 for one leaf: its distance, None when culled (the arithmetic of oracle/tree_oracle.py::gather)"""
    x, y, z = leaf["center"]
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
    dx, dy, dz = (leaf["max"][k] - leaf["min"][k] for k in range(3))
    ns = math.sqrt(dx * dx + dy * dy + dz * dz)
    out = -yz_z < (cos_y - .6) or -xz_z < (cos_x - .6)
    return None if (not gather_all and out and dist > ns) else dist


def gather(name, pose, base, transforms=None, mutation=None):
    """uint32 indexesToSort[0:splatRenderCount] of one pose; transforms None = the case's, mutation None = the feature as specified"""
    assert mutation is None or mutation in MUTATIONS
    case = cases.make_case(name)
    transforms = case["transforms"] if transforms is None else transforms
    base = [float(v) for v in base]
    if mutation == "mesh_world_in_base":
        base = multiply(base, case["mesh_world"])
    focal = (pose["height"] / 2.0) / math.tan(pose["fov"] / 2.0 * (math.pi / 180.0))
    cos_x = math.cos(math.atan(pose["width"] / 2.0 / focal))
    cos_y = math.cos(math.atan(pose["height"] / 2.0 / focal))
    ranges = cases.scene_ranges(case)
    kept, flat = [], 0
    for s, leaves in enumerate(sub_trees(name)):
        t = transforms[0 if mutation == "scene0_matrix" else s]
        mv = multiply(t, base) if mutation == "transform_times_base" else multiply(base, t)
        for local, leaf in enumerate(leaves):
            d = leaf_key(leaf, mv, cos_x, cos_y, pose["gather_all"])
            if d is not None:
                idx = leaf["indexes"] if mutation != "local_indexes" else [i - ranges[s][0] for i in leaf["indexes"]]
                kept.append((d, local if mutation == "tie_by_local_leaf" else flat, flat, idx))
            flat += 1
    kept.sort(key=lambda q: q[:3])
    out = []
    for q in reversed(kept):                                # the nearest leaf ends the buffer
        out.extend(q[3])
    return np.array(out, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def model_lists(name):
    """The model's list at every pose of the case's script (computed once, shared; callers must not change them)"""
    out = []
    for k, pose in enumerate(cases.make_script(name)):
        lst = gather(name, pose, golden_base(name, k))
        lst.setflags(write=False)
        out.append(lst)
    return out
