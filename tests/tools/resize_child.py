"""Child process of tests/test_gpu_mesh_resize.py::test_under_poisoned_allocations_in_a_child_process: a mesh and its bound sorter
are resized up, receive a further scene, draw, run a visibility-culled sort, are resized down and draw again - each step compared
with a fresh mesh and sorter of that capacity, every object created under whatever $GSPLAT_POISON_ALLOC the parent set.  Prints
`resize_child: ok` as its last line; a failed comparison raises."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gaussiansplats3d_amd import Context, camera, create_sort_worker, util  # noqa: E402
from test_gpu_mesh_remove import CONFIGS, new_mesh, same_as_fresh, scene_data, upload_runs  # noqa: E402
from test_gpu_sorter_remove import sort_list, upload  # noqa: E402


def pair(ctx, capacity, cfg, runs):
    mesh, worker = new_mesh(ctx, capacity, cfg), create_sort_worker(ctx, capacity)
    upload_runs(mesh, runs)
    upload(worker, [r[0] for r in runs], [0] * len(runs), True)
    return mesh, worker


def culled_frame(mesh, worker, mvp, n):
    """project, a visibility-culled sort whose list also comes to the host, the draw from the resident result"""
    worker.set_visibility_cull(True)
    mesh.use_sorter_result(worker, n)                      # binds
    mesh.project()
    kept = sort_list(worker, mvp, n)
    mesh.use_sorter_result(worker, n)
    frame = mesh.render()[0]
    worker.set_visibility_cull(False)
    return kept.tobytes(), frame.tobytes()


def main():
    ctx = Context(0)
    mvp = camera.demo_camera("garden", 64, 64).sort_mvp()
    for name in ("sh2_fp16", "sh2_fp32_u8"):
        cfg = CONFIGS[name]
        runs = [scene_data(n, cfg["deg"], 40 + k, cfg["u8"]) for k, n in enumerate((300, 257, 443))]
        mesh, worker = pair(ctx, 557, cfg, runs[:2])
        assert culled_frame(mesh, worker, mvp, 557)[1]     # (a draw and a sort before: buffers in use, caches warm)
        # up, the third scene, a draw
        mesh.resize(1400)
        worker.resize(1400)
        mesh.build(*runs[2], start=557)
        worker.post_message({"centers": util.integer_centers(runs[2][0]), "range": {"from": 557, "to": 999, "count": 443}})
        fresh_mesh, fresh_worker = pair(ctx, 1400, cfg, runs)
        same_as_fresh(mesh, fresh_mesh, 1400)
        assert culled_frame(mesh, worker, mvp, 1000) == culled_frame(fresh_mesh, fresh_worker, mvp, 1000)
        fresh_mesh.dispose()
        fresh_worker.terminate()
        # down to what is uploaded, another draw
        worker.resize(1000)
        mesh.resize(1000)
        fresh_mesh, fresh_worker = pair(ctx, 1000, cfg, runs)
        same_as_fresh(mesh, fresh_mesh, 1000)
        assert culled_frame(mesh, worker, mvp, 1000) == culled_frame(fresh_mesh, fresh_worker, mvp, 1000)
        for o in (worker, fresh_worker):
            o.terminate()
        for o in (mesh, fresh_mesh):
            o.dispose()
    ctx.close()
    print("resize_child: ok")


if __name__ == "__main__":
    main()
