"""The cases of tests/test_gpu_sort_plan.py whose switch is read once per process, in a process of their own: a sort per size against
the sort oracle, the executed inputs (gs_sorter_debug_read, selector 5) showing the switch and the executed plan equal to the host
model's.

usage: GSPLAT_TREE_NO_FUSE=1 | GSPLAT_NO_SORT_PACK=1 | GSPLAT_NO_SORT_CHUNK=1  python tests/tools/sort_plan_child.py SWITCH
       -> "sort_plan_child SWITCH: ok"; an exception (exit status 1) on a failure"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import known_range_cases as kr  # noqa: E402
import oracle  # noqa: E402
import sort_plan_cases as sc  # noqa: E402
import sort_plan_ref as ref  # noqa: E402
from gaussiansplats3d_amd import Context, camera, create_sort_worker, util  # noqa: E402

switch = sys.argv[1]
assert os.environ.get(switch), "the switch has to be set in the environment"
ctx = Context(0)
SIZES = (4097, 3 * 4096 * 2 + 1)
if switch == "GSPLAT_TREE_NO_FUSE":
    import helpers
    from oracle import tree_oracle
    from gaussiansplats3d_amd import SplatTree
    n = SIZES[1]
    c = helpers.small_scene(n, 0, seed=n).centers
    ci = util.integer_centers(c)
    cam = camera.demo_camera("garden", 640, 360)
    tree = SplatTree(ctx, 8, 200).process_splat_mesh(c)
    leaves, _ = tree_oracle.build_tree(c, None, 8, 200)
    idx = tree_oracle.gather(leaves, cam.view, 50.0, 640, 360)
    w = create_sort_worker(ctx, n)
    w.post_message({"centers": ci, "range": {"from": 0, "to": n - 1, "count": n}})
    tree.gather_scene_nodes_for_sort(cam, sort_worker=w, to_host=False)
    reply = w.sort_gathered(cam.sort_mvp())
    np.testing.assert_array_equal(reply["sortedIndexes"], oracle.sort_indexes(idx, ci, cam.sort_mvp()))
    sc.check_executed(w, switch, sw_tree_no_fuse=1, list=ref.LIST_DEVICE, pending_gather=1, gather=ref.GATHER_PLAIN, front=ref.FRONT_KEY_IDX,
                      own_payloads=0)
    w.terminate()
    tree.dispose()
else:
    no_pack = switch == "GSPLAT_NO_SORT_PACK"
    for n in SIZES:
        for precision in (16, 20):
            ci = kr.gaussian_centers(n, seed=n + precision)
            w = create_sort_worker(ctx, n, splat_sort_distance_map_precision=precision)
            kr.upload(w, ci)
            kr.check_sort(w, ci, kr.camera_mvp(1), kr.KNOWN, precision=precision, what=switch)
            i, pl = sc.check_executed(w, switch, precision=precision, uploaded=n, p0_chunked=0, p0_grid=ref.radix_grid_for(n), p0_skip_hist=1,
                                      **{"sw_" + ("no_pack" if no_pack else "no_chunk"): 1})
            outs = tuple(p["out"] for p in pl["pass"][:pl["passes"]])
            if no_pack:
                assert outs == ((ref.OUT_KV16, ref.OUT_FINAL) if precision == 16 else (ref.OUT_KV32, ref.OUT_KV32, ref.OUT_FINAL)), outs
            else:
                assert outs == ((ref.OUT_PACKED, ref.OUT_FINAL) if precision == 16 else (ref.OUT_PACKED, ref.OUT_PACKED, ref.OUT_FINAL)), outs
                assert all(p["chunked"] == 0 for p in pl["pass"])
            w.terminate()
ctx.close()
print(f"sort_plan_child {switch}: ok")
