"""-m gpu: what a gather hands a sorter (csrc/gather_plan.hpp, the hand-over record) through three ordinary life-cycle sequences
on the device - the numbering forgotten under a planned gather, the sorter destroyed under one, a tree without leaves.  Every
expected list is the oracle's gather (oracle/tree_oracle.py) sorted by the oracle's sorter, never the library's.  The scene is
tree_cases' clusters40k at 300 centres per node: leaves longer than one 256-entry round of the fused copy."""
import numpy as np
import pytest

import helpers
import oracle
import sort_plan_cases as sc
import sort_plan_ref as plan_ref
import tree_cases
from gaussiansplats3d_amd import Context, GsError, SplatMesh, SplatTree, camera, create_sort_worker, util
from oracle import tree_oracle

pytestmark = pytest.mark.gpu
EXTRA = 256                                                # a second, small scene behind the tree's splats: the one that is removed


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The scene, one camera, and the oracle's lists for it - computed once, read by every test."""
    c = tree_cases.make_case("clusters40k")["centers"]
    cam = camera.demo_camera("garden", 1280, 720)
    ci = util.integer_centers(c)
    leaves, _ = tree_oracle.build_tree(c, None, 8, 300)
    gathered = tree_oracle.gather(leaves, cam.view, 50.0, 1280, 720)
    assert 0 < len(gathered) < len(c) and max(len(lf["indexes"]) for lf in leaves) > 256
    out = dict(centers=c, ci=ci, cam=cam, mvp=cam.sort_mvp(), gathered=gathered, sorted=oracle.sort_indexes(gathered, ci, cam.sort_mvp()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def worker_with(ctx, want, extra=None):
    n = len(want["centers"])
    w = create_sort_worker(ctx, n + EXTRA)
    w.post_message({"centers": want["ci"], "range": {"from": 0, "to": n - 1, "count": n}})
    if extra is not None:
        w.post_message({"centers": util.integer_centers(extra), "range": {"from": n, "to": n + EXTRA - 1, "count": EXTRA}})
    return w


def planned_gather(tree, want, w, **kw):
    r = tree.gather_scene_nodes_for_sort(want["cam"], sort_worker=w, to_host=False, **kw)
    assert r["splatRenderCount"] == (len(want["centers"]) if kw.get("asynchronous") else len(want["gathered"]))


def sorts_to_the_oracles_list(want, w, planned):
    reply = w.sort_gathered(want["mvp"])
    assert reply["stats"].result_count == len(want["sorted"])
    np.testing.assert_array_equal(reply["sortedIndexes"][:len(want["sorted"])], want["sorted"])   # (beyond an asynchronous list's length: undefined)
    # the sort found the gather as the gather left it: still planned in the tree (copied by the key kernel), or already copied
    sc.check_executed(w, list=plan_ref.LIST_DEVICE, pending_gather=int(planned), gather=plan_ref.GATHER_FUSED if planned else plan_ref.GATHER_NONE)


def test_numbering_forgotten_under_a_planned_gather(ctx, want):
    c, n = want["centers"], len(want["centers"])
    body, tail = helpers.small_scene(n, 0, 5), helpers.small_scene(EXTRA, 0, 6)
    mesh = SplatMesh(ctx, n + EXTRA, 0)
    mesh.build(c, body.cov, body.rgba, None, start=0)
    mesh.build(tail.centers, tail.cov, tail.rgba, None, start=n)
    w = worker_with(ctx, want, tail.centers)
    tree = SplatTree(ctx, 8, 300).process_splat_mesh(c)
    try:
        mesh.set_camera(want["cam"])
        mesh.use_sorter_result(w, n + EXTRA)                 # binds
        planned_gather(tree, want, w)
        sorts_to_the_oracles_list(want, w, planned=True)     # (a gather into this sorter is a planned one)
        planned_gather(tree, want, w)
        mesh.remove([(n, EXTRA)])                            # the bound mesh renumbers: the sorter forgets every list that names splats
        with pytest.raises(GsError, match="no gs_tree_gather has filled"):
            w.sort_gathered(want["mvp"])
        w.remove([(n, EXTRA)])
        with pytest.raises(GsError, match="no gs_tree_gather has filled"):
            w.sort_gathered(want["mvp"])
        planned_gather(tree, want, w)                        # the tree's splats kept their numbers: a fresh gather sorts as ever
        sorts_to_the_oracles_list(want, w, planned=True)
    finally:
        tree.dispose(); w.terminate(); mesh.dispose()


def test_sorter_destroyed_under_a_planned_gather(ctx, want):
    tree = SplatTree(ctx, 8, 300).process_splat_mesh(want["centers"])
    first, second = worker_with(ctx, want), worker_with(ctx, want)
    try:
        planned_gather(tree, want, first)
        first.terminate()                                    # the tree must not remember it
        planned_gather(tree, want, second)
        sorts_to_the_oracles_list(want, second, planned=True)
        planned_gather(tree, want, second)
        host = tree.gather_scene_nodes_for_sort(want["cam"])  # to the host: the second sorter copies its planned list first
        np.testing.assert_array_equal(host["indexesToSort"], want["gathered"])
        sorts_to_the_oracles_list(want, second, planned=False)
    finally:
        tree.dispose(); first.terminate(); second.terminate()


@pytest.mark.parametrize("asynchronous", [False, True], ids=["synchronous", "count_on_device"])
def test_a_tree_without_leaves(ctx, want, asynchronous):
    c = want["centers"]
    empty = SplatTree(ctx, 8, 300).process_splat_mesh(c[:1000], alphas=np.zeros(1000, np.uint8), min_alpha=1)
    tree = SplatTree(ctx, 8, 300).process_splat_mesh(c)
    w = worker_with(ctx, want)
    try:
        assert empty.info().leaves == 0 and empty.info().splats == 0
        planned_gather(tree, want, w)                        # a plan in another tree: the empty gather supersedes it
        r = empty.gather_scene_nodes_for_sort(want["cam"], sort_worker=w, to_host=False, asynchronous=asynchronous)
        assert r["splatRenderCount"] == 0
        reply = w.sort_gathered(want["mvp"])
        assert reply["sortedIndexes"].size == 0 and reply["stats"].result_count == 0
        planned_gather(tree, want, w, asynchronous=asynchronous)
        sorts_to_the_oracles_list(want, w, planned=True)
    finally:
        empty.dispose(); tree.dispose(); w.terminate()
