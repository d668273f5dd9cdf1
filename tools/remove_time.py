"""What removing a scene costs (information, not a gate): three scenes of the C3 stand-in, 5.8 M splats in total,
live in one mesh and one sorter; the middle one goes.  Timed on one machine, after a warm-up, several repetitions, median and
spread:
  remove   gs_mesh_remove, then gs_sorter_remove: the two C calls themselves, each on its own clock
  rebuild  the alternative: destroy both, create a fresh mesh and sorter, upload the two survivors from host arrays
Both calls wait for the object's streams before they move anything and again before they return, so the host's clock around a
call is the clock of the work it enqueues (the state before each repetition is rebuilt outside the clock).  python tools/remove_time.py [--splats N] [--reps K] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussiansplats3d_amd import Context, SplatMesh, create_sort_worker, scenes, util  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=5_800_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    whole = scenes.make_config_scene("C3", args.splats)
    n = whole.count
    cuts = [0, n // 3, 2 * n // 3, n]
    parts = [(whole.centers[a:b], whole.cov[a:b], whole.rgba[a:b], whole.sh[a:b]) for a, b in zip(cuts, cuts[1:])]
    ints = [util.integer_centers(p[0]) for p in parts]
    ctx = Context(0)

    def build(which):
        mesh = SplatMesh(ctx, n, whole.sh_degree, half_precision_covariances=whole.cov_half)
        worker = create_sort_worker(ctx, n)
        at = 0
        for k in which:
            c = parts[k]
            mesh.build(*c, start=at)
            worker.post_message({"centers": ints[k], "range": {"from": at, "to": at + len(c[0]) - 1, "count": len(c[0])}})
            at += len(c[0])
        return mesh, worker

    gone = np.array([[cuts[1], cuts[2] - cuts[1]]], np.uint32)
    lib = ctx.lib
    t_mesh, t_sorter, t_rebuild = [], [], []
    for rep in range(args.reps + 1):                       # (the first repetition warms up and is dropped)
        mesh, worker = build([0, 1, 2])
        t0 = time.perf_counter()
        st_mesh = lib.gs_mesh_remove(mesh.handle, gone.ctypes.data, 1, None, 0)
        t1 = time.perf_counter()
        st_sorter = lib.gs_sorter_remove(worker.handle, gone.ctypes.data, 1, None, 0)
        t2 = time.perf_counter()
        assert st_mesh == 0 and st_sorter == 0, (st_mesh, st_sorter)
        mesh.dispose()
        worker.terminate()
        mesh, worker = build([0, 1, 2])
        t3 = time.perf_counter()
        mesh.dispose()
        worker.terminate()
        mesh, worker = build([0, 2])
        t4 = time.perf_counter()
        mesh.dispose()
        worker.terminate()
        if rep:
            t_mesh.append((t1 - t0) * 1e3)
            t_sorter.append((t2 - t1) * 1e3)
            t_rebuild.append((t4 - t3) * 1e3)
    ctx.close()
    spread = lambda t: {"median": statistics.median(t), "min": min(t), "max": max(t)}
    row = {"splats": n, "removed": int(gone[0][1]), "reps": args.reps, "gs_mesh_remove_ms": spread(t_mesh),
           "gs_sorter_remove_ms": spread(t_sorter), "destroy_and_rebuild_ms": spread(t_rebuild)}
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
