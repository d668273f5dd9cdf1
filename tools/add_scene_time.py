"""What adding a scene costs (information, not a gate): two scenes of the C3 stand-in, 3.9 M splats of SH degree 2,
live in one mesh and one sorter whose capacity is theirs; a third of 1.93 M is added.  Timed on one machine, after a warm-up,
several repetitions, median and spread, the host's clock around each C call:
  add      gs_mesh_resize, then the upload of the third scene; gs_sorter_resize, then the third scene's centres
  rebuild  the alternative: destroy both, create a fresh mesh and sorter of the full capacity, upload all three scenes from host
           arrays (the drop-in's host fills of every scene, which come before this in a Viewer, are not in the figure)
Every call waits for the object's streams before it moves anything and again before it returns, so the host's clock around a call
is the clock of the work it enqueues (the state before each repetition is rebuilt outside the clock).
python tools/add_scene_time.py [--splats N] [--reps K] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

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

    def upload(mesh, worker, k):
        c, at = parts[k], cuts[k]
        mesh.build(*c, start=at)
        worker.post_message({"centers": ints[k], "range": {"from": at, "to": at + len(c[0]) - 1, "count": len(c[0])}})

    def build(which, capacity):
        mesh = SplatMesh(ctx, capacity, whole.sh_degree, half_precision_covariances=whole.cov_half)
        worker = create_sort_worker(ctx, capacity)
        for k in which:
            upload(mesh, worker, k)
        return mesh, worker

    t = {name: [] for name in ("gs_mesh_resize_ms", "mesh_upload_ms", "gs_sorter_resize_ms", "sorter_centers_ms", "add_total_ms", "destroy_and_rebuild_ms")}
    for rep in range(args.reps + 1):                       # (the first repetition warms up and is dropped)
        mesh, worker = build([0, 1], cuts[2])
        t0 = time.perf_counter()
        mesh.resize(n)
        t1 = time.perf_counter()
        mesh.build(*parts[2], start=cuts[2])
        t2 = time.perf_counter()
        worker.resize(n)
        t3 = time.perf_counter()
        worker.post_message({"centers": ints[2], "range": {"from": cuts[2], "to": n - 1, "count": n - cuts[2]}})
        t4 = time.perf_counter()
        assert mesh.max_splat_count == n and mesh.splat_count == n and worker.uploaded_splat_count == n
        # the only path without the two calls: from two live scenes to three through destroy, create and three uploads
        t5 = time.perf_counter()
        mesh.dispose()
        worker.terminate()
        mesh, worker = build([0, 1, 2], n)
        t6 = time.perf_counter()
        mesh.dispose()
        worker.terminate()
        if rep:
            for name, ms in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0, t6 - t5)):
                t[name].append(ms * 1e3)
    ctx.close()
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    row = {"splats": n, "resident": cuts[2], "added": n - cuts[2], "sh_degree": whole.sh_degree, "reps": args.reps}
    row.update({name: spread(v) for name, v in t.items()})
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
