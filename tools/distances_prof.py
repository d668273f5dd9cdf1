"""The gpuAcceleratedSort distance pass at 5.8 M splats (the C3 count), for a rocprofv3 kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/distances_prof.py morton|keep [routes]
20 launches of gs_mesh_compute_distances per permutation (integer / float x static / dynamic) on a Morton-ordered or a
GS_MESH_KEEP_ORDER mesh of random centres; with `routes`, also the wall clock of distance pass + full sort through the host
(distances copied out and back in) against the device hand-over (dst + GS_PRECOMPUTED_DEVICE), 20 frames each, twice."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiansplats3d_amd import Context, SplatMesh, camera
from gaussiansplats3d_amd.sort_worker import SortWorker

N = 5_800_000
layout = sys.argv[1]
ctx = Context(0)
rng = np.random.default_rng(7)
cam = camera.demo_camera("garden", 1920, 1080)
pos = np.asarray(cam.position, np.float64)
centers = (pos + rng.normal(size=(N, 3)) * 4.0).astype(np.float32)
m = SplatMesh(ctx, N, keep_order=(layout == "keep"), dynamic_mode=True)
m.build(centers, np.zeros((N, 6), np.float32), np.zeros((N, 4), np.uint8), scene_indexes=(np.arange(N) % 3).astype(np.uint32))
m.set_scenes(transforms=[np.eye(4).reshape(16)] * 3)
mvp = np.asarray(cam.sort_mvp(), np.float64).reshape(16)
for integer in (True, False):
    for dynamic in (False, True):
        for _ in range(20):
            m.compute_distances_on_gpu(mvp, integer=integer, dynamic=dynamic)
        ctx.synchronize()
if len(sys.argv) > 2:
    for integer in (True, False):
        w = SortWorker(ctx, N, integer, False)
        w.set_uploaded_count(N)
        host = np.empty(N, np.int32 if integer else np.float32)
        base = {"modelViewProj": mvp, "splatRenderCount": N, "splatSortCount": N, "usePrecomputedDistances": True, "keepOnDevice": True}
        for route in ("host", "device", "host", "device"):
            ts = []
            for _ in range(20):
                t0 = time.perf_counter()
                if route == "host":
                    m.compute_distances_on_gpu(mvp, out=host, integer=integer, dynamic=False)
                    w.post_message({"sort": dict(base, precomputedDistances=host)})
                else:
                    m.compute_distances_on_gpu(mvp, sort_worker=w, integer=integer, dynamic=False)
                    w.post_message({"sort": dict(base, precomputedOnDevice=True)})
                ctx.synchronize()
                ts.append(time.perf_counter() - t0)
            print(f"route={route} integer={integer} median_ms={1e3 * float(np.median(ts)):.3f} min_ms={1e3 * min(ts):.3f}", flush=True)
        w.terminate()
m.dispose()
ctx.close()
print("PROF_OK")
