"""The octree gather's plan ON THE DEVICE (csrc/tree.hip: k_tree_test, k_tree_scan, k_tree_fill, k_tree_offsets), where leaves
share buckets: every step of every script of tests/tree_plan_cases.py, played IN ORDER on ONE device-built tree per test (the
tables the kernels carry from gather to gather - fill, hist, the previous keys, prev_scale - are the subject), against
oracle/tree_oracle.py::gather for splatRenderCount and the list, bit for bit, through the gather's three consumers:
  (i)   the synchronous gather with a host list (the script twice through on the same tree);
  (ii)  a static integer sort worker with the deferred, fused copy (sorter.hip, k_tree_copy_keys) against oracle.sort_indexes on
        the oracle's list; every third step a partial sort comes first (the plain copy);
  (iii) the asynchronous gather, without and with the per-splat frustum cull (oracle.culled_sort; its keep words are zeroed by
        k_tree_offsets);
and two sorters that alternate on one tree, each sorting only after the other's next gather has overwritten the plan.
The host model of the same kernels, its mutations and the properties of the case list: tests/test_tree_plan_ref.py."""
import numpy as np
import pytest

import tree_plan_cases as cases
from gaussiansplats3d_amd import SplatTree, create_sort_worker, util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gaussiansplats3d_amd import Context
    c = Context(0)
    yield c
    c.close()


class _Dims:
    def __init__(self, step):
        self.width, self.height = step["width"], step["height"]


def _device_tree(ctx, name):
    """One device-built tree of the scene; its leaves are the oracle's (so the host restatement's occupancies hold for it)."""
    scene = cases.make_scene(name)
    tree = SplatTree(ctx, scene["max_depth"], scene["max_centers"]).process_splat_mesh(scene["centers"])
    leaves = cases.oracle_leaves(name)
    _, centers, _, offsets, indexes = tree.leaves()
    np.testing.assert_array_equal(centers, np.array([lf["center"] for lf in leaves]).reshape(-1, 3))
    np.testing.assert_array_equal(indexes, np.concatenate([lf["indexes"] for lf in leaves]))
    np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)), [len(lf["indexes"]) for lf in leaves])
    return tree


def _worker(ctx, name):
    c = cases.make_scene(name)["centers"]
    ci = util.integer_centers(c)
    w = create_sort_worker(ctx, len(c))
    w.post_message({"centers": ci, "range": {"from": 0, "to": len(c) - 1, "count": len(c)}})
    return w, ci


def _gather(tree, step, **kw):
    return tree.gather_scene_nodes_for_sort(_Dims(step), gather_all_nodes=step["gather_all"], fov_deg=step["fov"],
                                            model_view=step["model_view"], **kw)


def _max_occupancy(name):
    return max(cases.step_report(name, k)["max_occupancy"] for k in range(len(cases.make_script(name))))


def _say(consumer, name, steps):
    print("\n%s, %s: %d steps on one device-built tree, largest bucket occupancy %d" % (consumer, name, steps, _max_occupancy(name)))


@pytest.mark.parametrize("name", cases.SCENES)
def test_synchronous_gather_follows_the_script_twice(ctx, name):
    script, want = cases.make_script(name), cases.oracle_lists(name)
    tree = _device_tree(ctx, name)
    steps = 0
    for lap in range(2):                                     # the second lap starts from the tables the first one left
        for k, s in enumerate(script):
            got = _gather(tree, s)
            where = "%s lap %d step %s" % (name, lap, s["tag"])
            assert got["splatRenderCount"] == len(want[k]), where
            np.testing.assert_array_equal(got["indexesToSort"], want[k], err_msg=where)
            steps += 1
    tree.dispose()
    _say("synchronous gather", name, steps)


@pytest.mark.parametrize("name", cases.SCENES)
def test_deferred_copy_of_a_static_sorter_follows_the_script(ctx, name):
    import oracle
    script, want = cases.make_script(name), cases.oracle_lists(name)
    tree = _device_tree(ctx, name)
    w, ci = _worker(ctx, name)
    for k, s in enumerate(script):
        where = "%s step %s" % (name, s["tag"])
        mvp = cases.sort_mvp(s)
        r = _gather(tree, s, sort_worker=w, to_host=False)
        R = r["splatRenderCount"]
        assert R == len(want[k]), where
        for sort_count in ((R // 3, R) if k % 3 == 2 else (R,)):      # Viewer.runSplatSort: partial sorts first, then the whole list
            reply = w.sort_gathered(mvp, sort_count)
            expect = oracle.sort_indexes(want[k], ci, mvp, sort_count=sort_count, render_count=R)
            np.testing.assert_array_equal(reply["sortedIndexes"], expect, err_msg="%s sort %d of %d" % (where, sort_count, R))
    w.terminate()
    tree.dispose()
    _say("deferred copy + static integer sort", name, len(script))


@pytest.mark.parametrize("frustum_cull", [False, True])
@pytest.mark.parametrize("name", cases.SCENES)
def test_asynchronous_gather_follows_the_script(ctx, name, frustum_cull):
    import oracle
    script, want = cases.make_script(name), cases.oracle_lists(name)
    tree = _device_tree(ctx, name)
    w, ci = _worker(ctx, name)
    w.set_frustum_cull(frustum_cull)
    splats = int(tree.info().splats)
    for k, s in enumerate(script):
        where = "%s step %s" % (name, s["tag"])
        mvp = cases.sort_mvp(s)
        r = _gather(tree, s, sort_worker=w, to_host=False, asynchronous=True)
        assert r["countOnDevice"] and r["splatRenderCount"] == splats
        w.sort_gathered(mvp, keep_on_device=True)
        st, _ = w.last_stats()
        if frustum_cull:
            expect, keep = oracle.culled_sort(want[k], ci, mvp)
            assert st.result_count == int(keep.sum()) == len(expect), where
        else:
            expect = oracle.sort_indexes(want[k], ci, mvp)
            assert st.result_count == len(want[k]), where
        if st.result_count:                                  # (positions beyond the result's length are undefined)
            np.testing.assert_array_equal(w.debug_read(2, int(st.result_count)), expect, err_msg=where)
    w.set_frustum_cull(False)
    w.terminate()
    tree.dispose()
    _say("asynchronous gather" + (" + frustum cull" if frustum_cull else ""), name, len(script))


@pytest.mark.parametrize("name", ["lat17", "lat257", "clusters10k"])
def test_two_sorters_alternate_on_one_tree(ctx, name):
    """Step k is gathered for sorter k % 2 and sorted only after step k + 1 has been gathered for the other sorter: that gather
    overwrites the plan's offsets, so the first sorter must have copied its list at that moment."""
    import oracle
    script, want = cases.make_script(name), cases.oracle_lists(name)
    tree = _device_tree(ctx, name)
    (w0, ci), (w1, _) = _worker(ctx, name), _worker(ctx, name)
    ws = (w0, w1)

    def check(k):
        mvp = cases.sort_mvp(script[k])
        reply = ws[k % 2].sort_gathered(mvp)
        np.testing.assert_array_equal(reply["sortedIndexes"], oracle.sort_indexes(want[k], ci, mvp),
                                      err_msg="%s step %s" % (name, script[k]["tag"]))

    for k, s in enumerate(script):
        r = _gather(tree, s, sort_worker=ws[k % 2], to_host=False)
        assert r["splatRenderCount"] == len(want[k]), (name, s["tag"])
        if k:
            check(k - 1)
    check(len(script) - 1)
    w0.terminate()
    w1.terminate()
    tree.dispose()
    _say("two alternating sorters", name, len(script))
