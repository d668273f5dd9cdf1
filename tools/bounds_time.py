"""Times one gs_mesh_bounds call over the 5.8 M-splat garden stand-in (the bench's C3 scene) next to its read floor: 16 bytes per
splat (px, py, pz, inv_perm) at the 8 TB/s HBM peak.  Information, not a gate: DESIGN 8.11 records the measured figure.

    python tools/bounds_time.py [--config C3] [--repeat 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from gaussiansplats3d_amd import Context, SplatMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    scene = scenes.make_config_scene(args.config)
    stream = torch.cuda.Stream()                            # the context's stream, so that torch events can bracket the call
    ctx = Context(0, stream=stream.cuda_stream, single_stream=True)
    mesh = SplatMesh(ctx, scene.count, 0)
    n = scene.count
    step = 1 << 20                                          # colour and covariance do not matter here: small constant arrays per upload
    cov, rgba = np.zeros((step, 6), np.float32), np.zeros((step, 4), np.uint8)
    for s in range(0, n, step):
        e = min(s + step, n)
        mesh.build(scene.centers[s:e], cov[:e - s], rgba[:e - s], start=s)
    center = scene.centers.mean(axis=0, dtype=np.float64)
    for _ in range(3):
        got = mesh.bounds(0, n, center)
    ctx.synchronize()
    # device time: an event pair on the context's stream around ONE call (the kernel and the copy of its partials); the call itself waits
    times = []
    for _ in range(args.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        mesh.bounds(0, n, center)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    floor_ms = 16.0 * n / 8e12 * 1e3
    print(json.dumps({"config": args.config, "splats": n, "uploads": (n + step - 1) // step, "bounds_ms_median": round(times[len(times) // 2], 4),
                      "bounds_ms_min": round(times[0], 4), "bounds_ms_max": round(times[-1], 4), "read_floor_ms_16B_per_splat_at_8TBs": round(floor_ms, 4),
                      "clock": "device events on the context's stream around one call, %d calls" % args.repeat,
                      "radius": float(np.sqrt(got["max_dist_sq"])), "count": got["count"]}))
    mesh.dispose()
    ctx.close()


if __name__ == "__main__":
    main()
