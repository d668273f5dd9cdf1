"""-m gpu: one small sort per front-end kind and per pass-chain shape.  After each sort gs_sorter_debug_read(what = 5) hands out
the inputs the sort was planned from and the plan that ran: the inputs are what the test arranged, the plan is what the host model
(sort_plan_ref.py) makes of those inputs, and the sorted list is the sort oracle's.  Switches that are read once per process run
in children (tools/sort_plan_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_cases
import known_range_cases as kr
import oracle
import sort_plan_cases as sc
import sort_plan_ref as ref
import vis_front_cases as vf
from gaussiansplats3d_amd import Context, camera, create_sort_worker, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 4097, 12289, 3 * 4096 * 2 + 1)                 # (the last: a chunk of the packed passes holds more than one tile)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def kat(ctx, what, cus, front, **case):
    """A sort of kat_cases' making through a fresh worker, against the oracle and the model."""
    case = dict(dict(name=what, precision=16, mode="int"), **case)
    case.setdefault("render", case["n"])
    case.setdefault("sort", case["render"])
    a = kat_cases.make_case(case)
    n = case["n"]
    w = create_sort_worker(ctx, n, True, True, a["use_int"], a["dynamic"], a["precision"])
    w.post_message({"centers": a["centers4"], "sceneIndexes": a["scene_indexes"], "range": {"from": 0, "to": n - 1, "count": n}})
    host_list = bool(case.get("permute"))
    reply = w.post_message({"sort": {"modelViewProj": a["mvp"], "splatRenderCount": a["render_count"], "splatSortCount": a["sort_count"],
                                     "usePrecomputedDistances": a["precomputed"] is not None, "indexesToSort": a["indexes"] if host_list else None,
                                     "transforms": a["transforms"], "precomputedDistances": a["precomputed"]}})
    kw = {k: a[k] for k in ("sort_count", "render_count", "precision", "use_int", "dynamic", "precomputed", "scene_indexes", "transforms")}
    np.testing.assert_array_equal(reply["sortedIndexes"], oracle.sort_indexes(a["indexes"], a["centers4"], a["mvp"], **kw), err_msg=what)
    sc.check_executed(w, what, flags=(1 if a["use_int"] else 0) | (2 if a["dynamic"] else 0), precision=a["precision"], uploaded=n,
                      sort_count=a["sort_count"], render_count=a["render_count"], list=ref.LIST_HOST if host_list else ref.LIST_IDENTITY,
                      precomputed=ref.PRE_HOST if a["precomputed"] is not None else ref.PRE_NONE, cu_count=cus, frustum_cull=0,
                      visibility_cull=0, count_on_device=0, pending_gather=0, mesh_map=0, front=front, known_range=0)
    w.terminate()


@pytest.mark.parametrize("n", SIZES)
def test_known_range_front_ends(ctx, cus, n):
    """Precision 16 with usable 16-bit planes (compact) and without (narrow), precision 20 (wide): twice each, so that pass 0's slot
    alternates; the host's key range is the oracle's."""
    for precision, scale, chain in ((16, 3000.0, (ref.OUT_PACKED, ref.OUT_FINAL)), (16, 30000.0, (ref.OUT_PACKED, ref.OUT_FINAL)),
                                    (20, 3000.0, (ref.OUT_PACKED, ref.OUT_PACKED, ref.OUT_FINAL))):
        ci = kr.gaussian_centers(n, seed=n + precision, scale=scale)
        fits = bool(((ci[:, :3].max(axis=0).astype(np.int64) - ci[:, :3].min(axis=0)) <= 65535).all())
        assert fits == (scale == 3000.0 or n == 1), "the wide scene is there to leave no usable 16-bit planes (one splat spans nothing)"
        front = ref.FRONT_KNOWN_WIDE if precision == 20 else ref.FRONT_KNOWN_COMPACT if fits else ref.FRONT_KNOWN_NARROW
        w = create_sort_worker(ctx, n, splat_sort_distance_map_precision=precision)
        kr.upload(w, ci)
        for k, slot in enumerate((3, 0)):
            sel = kr.check_sort(w, ci, kr.camera_mvp(k), kr.KNOWN, precision=precision, what=f"p{precision} scale {scale}")
            i, pl = sc.check_executed(w, f"n {n} p{precision}", flags=1, precision=precision, uploaded=n, sort_count=n, render_count=n, list=0,
                                      clean_slot=slot, extreme_current=1, c16_current=int(fits), range_ok=1, range_lo=int(sel[2]),
                                      range_hi=int(sel[3]), cu_count=cus, front=front, pass0_slot=slot, p0_skip_hist=1)
            assert tuple(p["out"] for p in pl["pass"][:pl["passes"]]) == chain
            assert pl["pass"][0]["chunked"] == 1 and pl["pass"][0]["grid"] == ref.radix_chunk_grid_for(n)
        w.terminate()


@pytest.mark.parametrize("n", SIZES[1:])
def test_key_kernel_front_ends(ctx, cus, n):
    """A partial sort, a host index list, and float, dynamic and precomputed sorters."""
    kat(ctx, "partial", cus, ref.FRONT_KEY_VEC4, n=n, sort=n // 3)
    kat(ctx, "host_list", cus, ref.FRONT_KEY_IDX, n=n, permute=True, render=n - 5, sort=n - 5)
    kat(ctx, "float_p20", cus, ref.FRONT_KEY_IDX, n=n, mode="float", precision=20)
    kat(ctx, "dynamic", cus, ref.FRONT_KEY_IDX, n=n, dynamic=True)
    kat(ctx, "precomputed", cus, ref.FRONT_KEY_IDX, n=n, precomputed=True)


@pytest.mark.parametrize("n", SIZES)
def test_frustum_cull_front_ends(ctx, cus, n):
    """The frustum cull on the identity list and on an index list."""
    ci = kr.gaussian_centers(n, seed=n, scale=3000.0)
    mvp = kr.camera_mvp(0)
    w = create_sort_worker(ctx, n)
    kr.upload(w, ci)
    w.set_frustum_cull(True)
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    for indexes, front, lst in ((None, ref.FRONT_CULL_VEC4, ref.LIST_IDENTITY), (perm, ref.FRONT_CULL_IDX, ref.LIST_HOST)):
        reply = w.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n, "indexesToSort": indexes}})
        kept_sorted, keep = oracle.culled_sort(np.arange(n, dtype=np.uint32) if indexes is None else indexes, ci, mvp)
        np.testing.assert_array_equal(reply["sortedIndexes"], kept_sorted)
        sc.check_executed(w, f"cull n {n}", frustum_cull=1, list=lst, uploaded=n, cu_count=cus, front=front, plan_count_on_device=1,
                          pass0_publishes=1, p0_in_cull=1, known_range=0)
    w.terminate()


@pytest.mark.parametrize("n", SIZES[1::2])
def test_visibility_cull_front_ends(ctx, cus, n):
    """The visibility cull after a full-frame projection (the streaming front end) and after a strip (the compacting one)."""
    rig = vf.Rig(ctx, n, vf.device_T())
    P = vf.pattern("rand30", n, rig.T)
    for strip, front in ((None, ref.FRONT_VIS_STREAM), (vf.STRIP, ref.FRONT_VIS_COMPACT), (None, ref.FRONT_VIS_STREAM)):
        assert rig.run(P, strip=strip, frame=False) == []      # (the list, the keep bits, min / max against the oracle)
        sc.check_executed(rig.worker, f"vis n {n} strip {strip}", visibility_cull=1, uploaded=n, sort_count=n, render_count=n, list=0,
                          mesh_map=1, mesh_uploaded=n, mesh_strip=int(strip is not None), cu_count=cus, front=front, vis_cull=1,
                          pass0_count=ref.COUNT_KEPT, plan_count_on_device=1, p0_in_idx=1)
    rig.close()


@pytest.mark.parametrize("n", SIZES[2:])
def test_gathered_lists(ctx, cus, n):
    """A planned gather the sort copies itself (fused), with and without the frustum cull, and an asynchronous gather, whose
    length stays on the device."""
    import helpers
    from oracle import tree_oracle
    from gaussiansplats3d_amd import SplatTree
    c = helpers.small_scene(n, 0, seed=n).centers
    ci = util.integer_centers(c)
    cam = camera.demo_camera("garden", 640, 360)
    tree = SplatTree(ctx, 8, 200).process_splat_mesh(c)
    leaves, _ = tree_oracle.build_tree(c, None, 8, 200)
    idx = tree_oracle.gather(leaves, cam.view, 50.0, 640, 360)
    expect = oracle.sort_indexes(idx, ci, cam.sort_mvp())
    kept_sorted, _ = oracle.culled_sort(idx, ci, cam.sort_mvp())
    w = create_sort_worker(ctx, n)
    w.post_message({"centers": ci, "range": {"from": 0, "to": n - 1, "count": n}})
    for cull, asynchronous in ((False, False), (True, False), (False, True), (True, True)):
        w.set_frustum_cull(cull)
        r = tree.gather_scene_nodes_for_sort(cam, sort_worker=w, to_host=False, asynchronous=asynchronous)
        R = r["splatRenderCount"]
        assert R == (int(tree.info().splats) if asynchronous else len(idx))
        w.sort_gathered(cam.sort_mvp(), keep_on_device=True)
        st, _ = w.last_stats()
        np.testing.assert_array_equal(w.debug_read(2, int(st.result_count)), kept_sorted if cull else expect)
        sc.check_executed(w, f"gather n {n} cull {cull} async {asynchronous}", list=ref.LIST_DEVICE, pending_gather=1, frustum_cull=int(cull),
                          pending_keep_zeroed=int(cull), count_on_device=int(asynchronous), render_count=R, sort_count=R, uploaded=n,
                          cu_count=cus, gather=ref.GATHER_FUSED, front=ref.FRONT_TREE_CULL if cull else ref.FRONT_TREE, own_payloads=1,
                          pass0_count=ref.COUNT_LIST if asynchronous else ref.COUNT_HOST, pass0_publishes=int(cull))
    # a partial sort of a planned gather: the plain copy, then the ordinary key kernel
    w.set_frustum_cull(False)
    tree.gather_scene_nodes_for_sort(cam, sort_worker=w, to_host=False)
    reply = w.sort_gathered(cam.sort_mvp(), len(idx) // 2)
    np.testing.assert_array_equal(reply["sortedIndexes"], oracle.sort_indexes(idx, ci, cam.sort_mvp(), sort_count=len(idx) // 2, render_count=len(idx)))
    sc.check_executed(w, "partial gather", list=ref.LIST_DEVICE, pending_gather=1, gather=ref.GATHER_PLAIN, front=ref.FRONT_KEY_IDX)
    w.terminate()
    tree.dispose()


CHILDREN = ("GSPLAT_TREE_NO_FUSE", "GSPLAT_NO_SORT_PACK", "GSPLAT_NO_SORT_CHUNK")


def test_switches_read_once_per_process():
    """A planned gather copied by the plain copy, the unpacked pass chains (16- and 32-bit keys + values) and the packed passes
    through the tile kernel: one child process per switch, all at once."""
    script = os.path.join(ROOT, "tests", "tools", "sort_plan_child.py")
    procs = [(sw, subprocess.Popen([sys.executable, script, sw], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   env=dict(os.environ, **{sw: "1"}))) for sw in CHILDREN]
    for sw, p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0 and f"sort_plan_child {sw}: ok" in out, out[-2000:]
