"""The per-scene octree cull of a dynamicMode mesh ON THE DEVICE (csrc/tree.hip: gs_tree_create_scenes, gs_tree_scene_leaves,
gs_tree_gather_scenes, k_tree_test_scenes): every pose of every script of tests/tree_scenes_cases.py, played IN ORDER on ONE tree
per test (the plan's tables carry over from gather to gather), against the recorded reference (tests/golden/tree_scenes_ref.json)
and the host model (tests/tree_scenes_ref.py), bit for bit, through
  (i)   the synchronous gather with a host list (the script twice through on the same tree);
  (ii)  the gather into a dynamic sort worker, then gs_sorter_sort_gathered, against oracle.sort_indexes with the scenes' transforms;
  (iii) the asynchronous gather, whose count stays on the device (a static worker: a sort that learns its length on the device is
        a full sort of a static scene), against oracle.sort_indexes on the reference's list;
  (iv)  two sort workers that alternate on one tree.
A tree of one scene must be gs_tree_create's, list for list; the flat leaf table must be the per-scene gs_tree_create trees one
after the other; every refusal returns its error and leaves the tree usable.  Host side of the same cases: test_tree_scenes_ref.py."""
import ctypes as C

import numpy as np
import pytest

import tree_scenes_cases as cases
import tree_scenes_ref as ref
from gaussiansplats3d_amd import GsError, SplatTree, create_sort_worker, util
from gaussiansplats3d_amd import _lib as L
from gaussiansplats3d_amd import camera as cam_math

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gaussiansplats3d_amd import Context
    c = Context(0)
    yield c
    c.close()


class _Dims:
    def __init__(self, pose):
        self.width, self.height = pose["width"], pose["height"]


def _tree(ctx, name):
    case = cases.make_case(name)
    return SplatTree(ctx, case["max_depth"], case["max_centers"]).process_splat_mesh_scenes(
        case["centers"], case["scene_counts"], case["alphas"], case["min_alphas"])


def _gather(tree, name, k, transforms=True, **kw):
    pose = cases.make_script(name)[k]
    return tree.gather_scene_nodes_for_sort(_Dims(pose), gather_all_nodes=pose["gather_all"], fov_deg=pose["fov"],
                                            model_view=ref.golden_base(name, k),
                                            scene_transforms=cases.make_case(name)["transforms"] if transforms else None, **kw)


def _want(name, k):
    """the recorded reference's list, which the host model reproduces (test_tree_scenes_ref.py holds that on the CPU too)"""
    want = ref.golden_list(name, k)
    np.testing.assert_array_equal(ref.model_lists(name)[k], want)
    return want


def _scene_indexes(case):
    return np.repeat(np.arange(len(case["scene_counts"]), dtype=np.uint32), case["scene_counts"])


def _worker(ctx, name):
    """a dynamic integer sort worker holding the case's centres and scene indexes"""
    case = cases.make_case(name)
    n = len(case["centers"])
    ci = util.integer_centers(case["centers"])
    w = create_sort_worker(ctx, n, dynamic_mode=True)
    w.post_message({"centers": ci, "sceneIndexes": _scene_indexes(case), "range": {"from": 0, "to": n - 1, "count": n}})
    return w, ci


def _sort_inputs(name, k):
    """(modelViewProj without the scenes' transforms, transforms fp32 [32 * 16]) of the sort that consumes pose k's list"""
    case, pose = cases.make_case(name), cases.make_script(name)[k]
    mvp = cam_math.multiply(cam_math.make_perspective(pose["fov"], pose["width"] / pose["height"], 0.1, 1000.0), ref.golden_base(name, k))
    tr = np.zeros(16 * L.GS_MAX_SCENES, np.float32)
    tr[:16 * len(case["transforms"])] = case["transforms"].astype(np.float32).reshape(-1)
    return mvp, tr


def _sorted_want(name, k, ci):
    import oracle
    mvp, tr = _sort_inputs(name, k)
    return oracle.sort_indexes(_want(name, k), ci, mvp, dynamic=True, scene_indexes=_scene_indexes(cases.make_case(name)), transforms=tr)


@pytest.mark.parametrize("name", cases.NAMES)
def test_leaf_table_is_the_scenes_own_trees_one_after_the_other(ctx, name):
    case = cases.make_case(name)
    keep = cases.keep_mask(case)
    tree = _tree(ctx, name)
    first = tree.scene_leaves()
    bounds, centers, depths, offsets, indexes = tree.leaves()
    assert first[0] == 0 and first[-1] == len(depths) == tree.info().leaves
    assert np.diff(first.astype(np.int64)).tolist() == ref.golden()[name]["subTreeLeaves"]
    for s, (a, b) in enumerate(cases.scene_ranges(case)):
        one = SplatTree(ctx, case["max_depth"], case["max_centers"]).process_splat_mesh(
            case["centers"][a:b], None if keep is None else keep[a:b].astype(np.uint8), 1, first_index=a)
        b1, c1, d1, o1, i1 = one.leaves()
        lo, hi = int(first[s]), int(first[s + 1])
        np.testing.assert_array_equal(bounds[lo:hi], b1)
        np.testing.assert_array_equal(centers[lo:hi], c1)
        np.testing.assert_array_equal(depths[lo:hi], d1)
        np.testing.assert_array_equal(offsets[lo:hi + 1].astype(np.int64) - int(offsets[lo]), o1)
        np.testing.assert_array_equal(indexes[offsets[lo]:offsets[hi]], i1)
        # ... and the host model's (oracle/tree_oracle.py::build_tree per scene)
        assert [lf["indexes"] for lf in ref.sub_trees(name)[s]] == [i1[o1[j]:o1[j + 1]].tolist() for j in range(len(d1))]
        one.dispose()
    tree.dispose()


@pytest.mark.parametrize("name", cases.NAMES)
def test_synchronous_gather_follows_the_script_twice(ctx, name):
    tree = _tree(ctx, name)
    for lap in range(2):                                     # the second lap starts from the tables the first one left
        for k, pose in enumerate(cases.make_script(name)):
            got = _gather(tree, name, k)
            where = "%s lap %d pose %s" % (name, lap, pose["tag"])
            assert got["splatRenderCount"] == len(_want(name, k)), where
            np.testing.assert_array_equal(got["indexesToSort"], _want(name, k), err_msg=where)
    tree.dispose()


@pytest.mark.parametrize("name", cases.NAMES)
def test_dynamic_sorter_sorts_the_gathered_list(ctx, name):
    tree = _tree(ctx, name)
    w, ci = _worker(ctx, name)
    for k, pose in enumerate(cases.make_script(name)):
        where = "%s pose %s" % (name, pose["tag"])
        r = _gather(tree, name, k, sort_worker=w, to_host=False)
        assert r["splatRenderCount"] == len(_want(name, k)), where
        mvp, tr = _sort_inputs(name, k)
        reply = w.sort_gathered(mvp, transforms=tr)
        np.testing.assert_array_equal(reply["sortedIndexes"], _sorted_want(name, k, ci), err_msg=where)
    w.terminate()
    tree.dispose()


def _static_worker(ctx, name):
    c = cases.make_case(name)["centers"]
    ci = util.integer_centers(c)
    w = create_sort_worker(ctx, len(c))
    w.post_message({"centers": ci, "range": {"from": 0, "to": len(c) - 1, "count": len(c)}})
    return w, ci


@pytest.mark.parametrize("name", cases.NAMES)
def test_asynchronous_gather_keeps_the_count_on_the_device(ctx, name):
    import oracle
    tree = _tree(ctx, name)
    w, ci = _static_worker(ctx, name)
    splats = int(tree.info().splats)
    for k, pose in enumerate(cases.make_script(name)):
        where = "%s pose %s" % (name, pose["tag"])
        r = _gather(tree, name, k, sort_worker=w, to_host=False, asynchronous=True)
        assert r["countOnDevice"] and r["splatRenderCount"] == splats
        mvp, _ = _sort_inputs(name, k)
        w.sort_gathered(mvp, keep_on_device=True)
        st, _ = w.last_stats()
        assert st.result_count == len(_want(name, k)), where
        if st.result_count:                                  # (positions beyond the result's length are undefined)
            np.testing.assert_array_equal(w.debug_read(2, int(st.result_count)), oracle.sort_indexes(_want(name, k), ci, mvp), err_msg=where)
    w.terminate()
    tree.dispose()


@pytest.mark.parametrize("name", ["three", "flat257", "max"])
def test_two_sorters_alternate_on_one_tree(ctx, name):
    """Pose k is gathered for sorter k % 2 and sorted only after pose k + 1 has been gathered for the other sorter."""
    tree = _tree(ctx, name)
    (w0, ci), (w1, _) = _worker(ctx, name), _worker(ctx, name)
    ws = (w0, w1)
    script = cases.make_script(name)

    def check(k):
        mvp, tr = _sort_inputs(name, k)
        reply = ws[k % 2].sort_gathered(mvp, transforms=tr)
        np.testing.assert_array_equal(reply["sortedIndexes"], _sorted_want(name, k, ci), err_msg="%s pose %s" % (name, script[k]["tag"]))

    for k in range(len(script)):
        r = _gather(tree, name, k, sort_worker=ws[k % 2], to_host=False)
        assert r["splatRenderCount"] == len(_want(name, k)), (name, script[k]["tag"])
        if k:
            check(k - 1)
    check(len(script) - 1)
    w0.terminate()
    w1.terminate()
    tree.dispose()


def test_static_sorter_gets_its_list_at_once(ctx):
    """A tree of several sub-trees never defers its copy to the sorter: a static worker's list is in place after the gather."""
    name = "two"
    tree = _tree(ctx, name)
    w, ci = _static_worker(ctx, name)
    r = _gather(tree, name, 0, sort_worker=w, to_host=False)
    assert r["splatRenderCount"] == len(_want(name, 0))
    # the next gather (no sorter) overwrites the plan; the worker's list must already be its own
    _gather(tree, name, 4)
    import oracle
    mvp, _ = _sort_inputs(name, 0)
    reply = w.sort_gathered(mvp)
    np.testing.assert_array_equal(reply["sortedIndexes"], oracle.sort_indexes(_want(name, 0), ci, mvp))
    w.terminate()
    tree.dispose()


@pytest.mark.parametrize("name", ["two", "flat257"])
def test_one_scene_is_the_plain_tree(ctx, name):
    """scene_count == 1: gs_tree_create + gs_tree_gather, leaf for leaf and list for list; its one transform multiplies the base."""
    case = cases.make_case(name)
    c = case["centers"]
    a = SplatTree(ctx, case["max_depth"], case["max_centers"]).process_splat_mesh_scenes(c, [len(c)])
    b = SplatTree(ctx, case["max_depth"], case["max_centers"]).process_splat_mesh(c)
    for x, y in zip(a.leaves(), b.leaves()):
        np.testing.assert_array_equal(x, y)
    assert a.scene_leaves().tolist() == b.scene_leaves().tolist() == [0, a.info().leaves]
    t = case["transforms"][1]
    for k, pose in enumerate(cases.make_script(name)):
        base = ref.golden_base(name, k)
        kw = dict(gather_all_nodes=pose["gather_all"], fov_deg=pose["fov"])
        ga = a.gather_scene_nodes_for_sort(_Dims(pose), model_view=base, **kw)
        gb = b.gather_scene_nodes_for_sort(_Dims(pose), model_view=base, **kw)
        np.testing.assert_array_equal(ga["indexesToSort"], gb["indexesToSort"])
        ga = a.gather_scene_nodes_for_sort(_Dims(pose), model_view=base, scene_transforms=[t], **kw)
        gb = b.gather_scene_nodes_for_sort(_Dims(pose), model_view=np.array(ref.multiply(base, t)), **kw)
        np.testing.assert_array_equal(ga["indexesToSort"], gb["indexesToSort"])
    a.dispose()
    b.dispose()


def test_plain_gather_on_a_tree_of_scenes_uses_the_base_for_every_scene(ctx):
    name = "three"
    case = cases.make_case(name)
    tree = _tree(ctx, name)
    eye = np.tile(cases.IDENTITY, (len(case["scene_counts"]), 1))
    for k, pose in enumerate(cases.make_script(name)):
        got = _gather(tree, name, k, transforms=False)
        want = ref.gather(name, pose, ref.golden_base(name, k), transforms=eye)
        np.testing.assert_array_equal(got["indexesToSort"], want, err_msg=pose["tag"])
    tree.dispose()


def test_refusals_name_their_reason_and_leave_the_tree_usable(ctx):
    name = "two"
    case = cases.make_case(name)
    tree = _tree(ctx, name)
    pose = cases.make_script(name)[0]
    kw = dict(gather_all_nodes=pose["gather_all"], fov_deg=pose["fov"], model_view=ref.golden_base(name, 0))
    for wrong in (1, 3):                                     # a transform count that is not the tree's scene count
        with pytest.raises(GsError) as e:
            tree.gather_scene_nodes_for_sort(_Dims(pose), scene_transforms=np.tile(cases.IDENTITY, (wrong, 1)), **kw)
        assert e.value.status == L.GS_ERR_INVALID and "%d scene transforms for a tree of 2 scenes" % wrong in str(e.value)
    host_only = SplatTree(None, case["max_depth"], case["max_centers"]).process_splat_mesh_scenes(case["centers"], case["scene_counts"])
    assert host_only.scene_leaves().tolist() == tree.scene_leaves().tolist()
    with pytest.raises(GsError) as e:                        # a tree without a context
        host_only.gather_scene_nodes_for_sort(_Dims(pose), scene_transforms=case["transforms"], **kw)
    assert e.value.status == L.GS_ERR_INVALID and "without a context" in str(e.value)
    host_only.dispose()
    lib, out = tree.lib, C.c_void_p()
    counts = np.ones(L.GS_MAX_SCENES + 1, np.uint32)
    pts = np.zeros((L.GS_MAX_SCENES + 1, 3), np.float32)
    for scene_count in (0, L.GS_MAX_SCENES + 1):
        assert lib.gs_tree_create_scenes(ctx.handle, pts.ctypes.data, None, scene_count, counts.ctypes.data, 2, 2, C.byref(out)) == L.GS_ERR_INVALID
        assert not out
    got = _gather(tree, name, 0)
    np.testing.assert_array_equal(got["indexesToSort"], _want(name, 0))
    tree.dispose()
