"""The per-scene octree cull of a dynamicMode mesh, on the host (no GPU): the model of tests/tree_scenes_ref.py against the recorded
reference (tests/golden/tree_scenes_ref.json: the reference's own worker and Viewer.gatherSceneNodesForSort text, dynamicMode: true),
bit for bit on every pose of every case, and the properties that give the case list its teeth.  Each way of getting the feature wrong
(tree_scenes_ref.MUTATIONS) must be caught by at least one recorded case; `scene0_matrix` - every leaf tested under scene 0's
transform - is what a single pooled tree does, so its failure is what separates the feature from the code before it.
The device against the same golden: tests/test_gpu_tree_scenes.py."""
import numpy as np
import pytest

import tree_scenes_cases as cases
import tree_scenes_ref as ref


def test_golden_covers_the_case_list():
    g = ref.golden()
    assert sorted(g) == sorted(cases.NAMES)
    for name in cases.NAMES:
        case = cases.make_case(name)
        assert g[name]["seed"] == case["seed"] and g[name]["splats"] == int(case["scene_counts"].sum()), name
        assert [p["tag"] for p in g[name]["poses"]] == [p["tag"] for p in cases.make_script(name)], name
        assert len(g[name]["subTreeLeaves"]) == len(case["scene_counts"]) == len(case["transforms"]), name
        if case["scene_leaves"] is not None:
            assert g[name]["subTreeLeaves"] == case["scene_leaves"], name


def test_case_list_has_the_shapes_the_kernel_can_go_wrong_at():
    g = ref.golden()
    leaves = {name: g[name]["subTreeLeaves"] for name in cases.NAMES}
    assert sorted(len(v) for v in leaves.values())[:1] == [2] and any(len(v) == 3 for v in leaves.values())
    assert len(leaves["max"]) == cases.MAX_SCENES == 32
    assert 1 in leaves["three"] and max(leaves["three"]) >= 300                  # a single leaf next to several hundred
    assert [sum(leaves[n]) for n in ("flat255", "flat256", "flat257")] == [255, 256, 257]
    assert leaves["flat257"][0] == 256                                          # a scene boundary on the 256-thread workgroup's edge
    assert 0 < leaves["flat255"][0] < 255                                       # ... and one inside a workgroup
    assert leaves["alpha"][1] == 0 and leaves["alpha"][0] > 0 and leaves["alpha"][2] > 0   # a filter that keeps nothing
    # a scene entirely culled and one entirely kept, then gatherAll
    case = cases.make_case("culled_kept")
    (a0, b0), (a1, b1) = cases.scene_ranges(case)
    ahead = ref.golden_list("culled_kept", 0)
    assert ahead.min() >= a1 and len(ahead) == b1 - a1
    assert len(ref.golden_list("culled_kept", 1)) == b1 - a0
    # every kind of transform occurs
    kinds = {"identity": 0, "translation": 0, "rotation": 0, "scale": 0}
    for name in cases.NAMES:
        for t in cases.make_case(name)["transforms"]:
            m = t.reshape(4, 4).T[:3, :3]
            if np.array_equal(t, cases.IDENTITY):
                kinds["identity"] += 1
            elif np.array_equal(m, np.eye(3)):
                kinds["translation"] += 1
            elif np.array_equal(m, np.diag(np.diag(m))):
                kinds["scale"] += 1
            else:
                kinds["rotation"] += 1
    assert all(kinds.values()), kinds
    # twins: the same points under the same transform
    tw = cases.make_case("twins")
    (a0, b0), (a1, b1) = cases.scene_ranges(tw)
    assert np.array_equal(tw["centers"][a0:b0], tw["centers"][a1:b1]) and np.array_equal(tw["transforms"][0], tw["transforms"][1])


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_builds_the_reference_sub_trees(name):
    assert [len(t) for t in ref.sub_trees(name)] == ref.golden()[name]["subTreeLeaves"]


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_equals_the_reference_on_every_pose(name):
    g = ref.golden()[name]
    for k, lst in enumerate(ref.model_lists(name)):
        where = "%s pose %s" % (name, g["poses"][k]["tag"])
        assert len(lst) == g["poses"][k]["splatRenderCount"], where
        np.testing.assert_array_equal(lst, ref.golden_list(name, k), err_msg=where)


def test_twins_tie_across_sub_trees_with_different_leaf_numbers():
    """At the `ties` pose leaves of the two sub-trees tie exactly, also where their numbers inside their sub-trees differ."""
    import math
    pose = cases.make_script("twins")[1]
    assert pose["tag"] == "ties"
    base = ref.golden_base("twins", 1)
    t0, t1 = ref.sub_trees("twins")
    key = lambda lf: ref.leaf_key(lf, ref.multiply(base, cases.IDENTITY), math.cos(0.5), math.cos(0.5), True)      # noqa: E731
    k0, k1 = [key(lf) for lf in t0], [key(lf) for lf in t1]
    assert k0 == k1
    assert sum(1 for i, a in enumerate(k0) for j, b in enumerate(k1) if a == b and j < i) > 0


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_every_mutation_is_caught_by_a_recorded_case(mutation):
    caught = []
    for name in cases.NAMES:
        for k, pose in enumerate(cases.make_script(name)):
            got = ref.gather(name, pose, ref.golden_base(name, k), mutation=mutation)
            if not np.array_equal(got, ref.golden_list(name, k)):
                caught.append((name, pose["tag"]))
    print("\n%s: caught by %d poses, first %s" % (mutation, len(caught), caught[:3]))
    assert caught, mutation
    if mutation == "tie_by_local_leaf":
        assert ("twins", "ties") in caught


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_only_library_tree_is_the_model_s_leaf_table(name):
    """gs_tree_create_scenes without a context (the recursive host builder): the sub-trees one after the other, global indexes."""
    from gaussiansplats3d_amd import SplatTree
    case = cases.make_case(name)
    tree = SplatTree(None, case["max_depth"], case["max_centers"]).process_splat_mesh_scenes(
        case["centers"], case["scene_counts"], case["alphas"], case["min_alphas"])
    subs = ref.sub_trees(name)
    flat = [lf for t in subs for lf in t]
    bounds, centers, depths, offsets, indexes = tree.leaves()
    assert np.diff(tree.scene_leaves().astype(np.int64)).tolist() == [len(t) for t in subs]
    np.testing.assert_array_equal(centers, np.array([lf["center"] for lf in flat]).reshape(-1, 3))
    np.testing.assert_array_equal(bounds, np.array([lf["min"] + lf["max"] for lf in flat]).reshape(-1, 6))
    np.testing.assert_array_equal(depths, [lf["depth"] for lf in flat])
    np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), [len(lf["indexes"]) for lf in flat])
    np.testing.assert_array_equal(indexes, np.concatenate([lf["indexes"] for lf in flat]))
    tree.dispose()
