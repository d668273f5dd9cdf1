"""-m gpu: the octree cull of a dynamicMode mesh through the JavaScript drop-in (node/SplatMesh.mjs, driven by
tests/tree_scenes_via_viewer.mjs).  A two-scene dynamic SplatMesh builds its tree with one sub-tree per scene; the Viewer's own
gatherSceneNodesForSort text walking HipSplatTree.subTrees with the mesh's getSceneTransform, the device-side HipSplatTree.gather
and the recorded reference (tests/golden/tree_scenes_ref.json, case `dropin`) give the same list at every pose.  At the pose
`toward1` a tree that tested scene 1's leaves under scene 0's transform would drop all of them: the frame drawn from the culled list
equals the frame drawn from the gatherAllNodes list (both in exact back-to-front order), and is not empty.  The Viewer's text comes from
oracle/_ref/seam/viewer_cut.json (made by the build where the reference is present); without it the device gather and the tree's
shape are still held to the reference."""
import json
import os
import shutil

import numpy as np
import pytest

import tree_scenes_cases as cases
import tree_scenes_ref as ref
from test_node_seam import BUNDLE, ROOT, _node

pytestmark = pytest.mark.gpu
NAME = "dropin"
W, H = 320, 180


def _back_to_front(case, cam, listed):
    """the listed splats by exact view depth, farthest first (ties by index): the same relative order for every list, so two frames
    differ only in which splats their lists hold"""
    scene = np.repeat(np.arange(len(case["scene_counts"])), case["scene_counts"])
    c = np.concatenate([case["centers"].astype(np.float64), np.ones((len(scene), 1))], axis=1)
    t = case["transforms"].reshape(-1, 4, 4).transpose(0, 2, 1)[scene]                       # column-major -> math matrices
    world = np.einsum("nij,nj->ni", t, c)
    z = (np.asarray(cam.view, np.float64).reshape(4, 4).T @ world.T)[2]
    listed = np.sort(np.asarray(listed, np.int64))
    return listed[np.argsort(z[listed], kind="stable")]


def test_two_scene_dynamic_mesh_culls_per_scene_through_the_drop_in(tmp_path):
    assert shutil.which("node") is not None, "node is part of the toolchain: the Node seam cannot go untested"
    case, script = cases.make_case(NAME), cases.make_script(NAME)
    assert (case["max_depth"], case["max_centers"]) == (8, 1000)          # what SplatMesh.buildSplatTree fixes
    job = {"scenes": [case["centers"][a:b].astype(np.float64).reshape(-1).tolist() for a, b in cases.scene_ranges(case)],
           "transforms": [t.tolist() for t in case["transforms"]], "meshWorld": case["mesh_world"].tolist(),
           "poses": [dict(matrixWorld=p["matrix_world"].tolist(), fov=p["fov"], width=p["width"], height=p["height"], gatherAll=p["gather_all"])
                     for p in script]}
    # the draw at `toward1`: eye at (20, 0, 0) looking at scene 1, 40 along x; scene 0 sits behind the eye
    from gaussiansplats3d_amd import camera
    assert script[0]["tag"] == "toward1" and script[3]["tag"] == "all" and script[3]["gather_all"]
    cam = camera.PerspectiveCamera(W, H, (20.0, 0.0, 0.0), (40.0, 0.0, 0.0), (0.0, 1.0, 0.0), fov=script[0]["fov"])
    np.testing.assert_array_equal(np.asarray(cam.matrix_world, np.float64).reshape(16), script[0]["matrix_world"])
    job["draw"] = {"width": W, "height": H, "focal": list(cam.focal(1.0)), "matrixWorld": np.asarray(cam.matrix_world, np.float64).reshape(-1).tolist(),
                   "view": np.asarray(cam.view, np.float64).reshape(-1).tolist(), "proj": np.asarray(cam.projection, np.float64).reshape(-1).tolist(),
                   "orders": {"culled": _back_to_front(case, cam, ref.golden_list(NAME, 0)).tolist(),
                              "all": _back_to_front(case, cam, ref.golden_list(NAME, 3)).tolist()}}
    (tmp_path / "in.json").write_text(json.dumps(job))
    have_text = os.path.exists(os.path.join(BUNDLE, "viewer_cut.json"))
    _node([os.path.join(ROOT, "tests", "tree_scenes_via_viewer.mjs"), BUNDLE if have_text else "-", str(tmp_path / "in.json"), str(tmp_path)],
          timeout=120)
    meta = json.load(open(tmp_path / "meta.json"))
    golden = ref.golden()[NAME]
    assert len(meta["subTrees"]) == len(case["scene_counts"]) == 2
    assert meta["subTrees"] == golden["subTreeLeaves"] and meta["visited"] == sum(golden["subTreeLeaves"]) <= meta["counted"]
    (a0, b0), (a1, b1) = cases.scene_ranges(case)
    for k, pose in enumerate(script):
        want = ref.golden_list(NAME, k)
        device = np.fromfile(tmp_path / ("device%d.u32" % k), dtype=np.uint32)
        assert meta["device"][k] == len(want), pose["tag"]
        np.testing.assert_array_equal(device, want, err_msg="device gather, pose " + pose["tag"])
        if have_text:
            walk = np.fromfile(tmp_path / ("walk%d.u32" % k), dtype=np.uint32)
            assert meta["walk"][k] == len(want), pose["tag"]
            np.testing.assert_array_equal(walk, want, err_msg="the Viewer's walk, pose " + pose["tag"])
    print("\nViewer text walked the drop-in tree: %s" % have_text)
    # `toward1`: scene 1 alone is kept; under scene 0's transform its leaves would sit behind the eye and all be dropped
    toward1 = ref.golden_list(NAME, 0)
    assert script[0]["tag"] == "toward1" and len(toward1) == b1 - a1 and toward1.min() >= a1
    assert len(ref.gather(NAME, script[0], ref.golden_base(NAME, 0), mutation="scene0_matrix")) == 0
    # ... and the frame with the tree on is the frame of gatherAllNodes
    culled = np.fromfile(tmp_path / "frame_culled.u8", np.uint8).reshape(H, W, 4)
    everything = np.fromfile(tmp_path / "frame_all.u8", np.uint8).reshape(H, W, 4)
    assert int((everything[..., :3].max(axis=2) > 0).sum()) > 100, "the frame of gatherAllNodes shows scene 1"
    assert np.array_equal(culled, everything), "the culled list must draw the frame of gatherAllNodes at this pose"

