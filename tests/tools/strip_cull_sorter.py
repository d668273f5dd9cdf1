"""The strip contract of tests/test_gpu_strip_cull.py through the sorter: per case of strip_cull_cases.SORTER_NAMES and per strip,
gs_mesh_project(strip) + a visibility-culled sort; the sorter's keep bits must equal strip_planes' mask of the full frame and the
sorted list the sort oracle's order restricted to it.  $GSPLAT_VIS_FRONT (read once per process) picks the front end.

usage: GSPLAT_VIS_FRONT=stream|compact python tests/tools/strip_cull_sorter.py   -> "strip_cull_sorter: N comparisons, 0 failures front=..." """
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle
import strip_cull_cases as cases
import strip_cull_ref as ref
from gaussiansplats3d_amd import Context, create_sort_worker, util

ctx = Context(0)
failures = comparisons = 0
for name in cases.SORTER_NAMES:
    case = cases.make_case(name)
    n = case.count
    mvp = case.cam.sort_mvp(case.mesh_world)
    with np.errstate(invalid="ignore"):
        ci = util.integer_centers(cases.final_centers(case))
    order = oracle.sort_indexes(np.arange(n, dtype=np.uint32), ci, mvp)
    mesh = cases.build_mesh(ctx, case)
    mesh.render()
    recs, rects, vis = mesh.debug_records()
    worker = create_sort_worker(ctx, n)
    worker.post_message({"centers": ci, "range": {"from": 0, "to": n - 1, "count": n}})
    mesh.use_sorter_result(worker, n)
    worker.set_visibility_cull(True)
    for strip in [None] + cases.STRIPS:
        want = vis if strip is None else ref.strip_planes(vis, rects, recs, *strip)[0]
        mesh.project(strip)
        reply = worker.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n}})
        bits = worker.keep_bits(n)
        _, st = mesh.render(tile_rows=strip)
        ok = (np.array_equal(bits, want) and np.array_equal(reply["sortedIndexes"], order[want[order]]) and
              int(reply["stats"].result_count) == int(st.visible_splats) == int(want.sum()))
        comparisons += 1
        if not ok:
            failures += 1
            print(f"FAIL {name} strip {strip}: keep bits differ at {np.nonzero(bits != want)[0][:5].tolist()}, "
                  f"kept {int(reply['stats'].result_count)} drawn {int(st.visible_splats)} expected {int(want.sum())}")
    worker.terminate()
    mesh.dispose()
ctx.close()
print(f"strip_cull_sorter: {comparisons} comparisons, {failures} failures front={os.environ.get('GSPLAT_VIS_FRONT', 'default')}")
sys.exit(1 if failures else 0)
