"""Times a full-frame surface pass (gs_mesh_surface, device outputs) next to the blend of the draw it reads, at the bench's C3
configuration (the garden stand-in at 1080p).  Information, not a gate: DESIGN records the measured pair.

    python tools/surface_time.py [--config C3] [--threshold 0.5] [--repeat 50]
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

    from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=50)
    args = ap.parse_args()
    cfg = scenes.CONFIGS[args.config]
    scene = scenes.make_config_scene(args.config)
    cam = camera.demo_camera(cfg["pose"], cfg["width"], cfg["height"])
    stream = torch.cuda.Stream()                            # the context's stream, so that torch events can bracket the pass
    ctx = Context(0, stream=stream.cuda_stream, single_stream=True)
    mesh = SplatMesh(ctx, scene.count, scene.sh_degree, scene.cov_half)
    mesh.build(scene.centers, scene.cov, scene.rgba, scene.sh if scene.sh_degree else None)
    worker = create_sort_worker(ctx, scene.count)
    worker.post_message({"centers": util.integer_centers(scene.centers), "range": {"from": 0, "to": scene.count - 1, "count": scene.count}})
    mesh.set_camera(cam)
    blend = []
    torch.cuda.synchronize()
    for _ in range(5):                                      # the list-bin size and the blend's bin order settle over a few draws
        worker.sort_on_device(cam.sort_mvp(), scene.count)
        mesh.use_sorter_result(worker, scene.count)
        _, stats = mesh.render(to_host=False)
        blend.append(float(stats.blend_ms))
    w, h = cam.width, cam.height
    ids = torch.empty((h, w), dtype=torch.int32, device="cuda")
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        mesh.surface(0, 0, w, h, args.threshold, ids_device_ptr=ids.data_ptr(), depth_device_ptr=depth.data_ptr())
    ctx.synchronize()
    # device time, like the draw's blend_ms: an event pair on the context's stream around the passes, enqueued back to back
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.repeat):
        mesh.surface(0, 0, w, h, args.threshold, ids_device_ptr=ids.data_ptr(), depth_device_ptr=depth.data_ptr())
    e1.record(stream)
    e1.synchronize()
    surface_ms = e0.elapsed_time(e1) / args.repeat
    hit = float((ids.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).mean())
    print(json.dumps({"config": args.config, "width": w, "height": h, "threshold": args.threshold, "blend_ms": round(blend[-1], 4),
                      "surface_ms": round(surface_ms, 4), "clock": "device events on the context's stream: blend_ms around one draw's blend, surface_ms over %d passes back to back" % args.repeat,
                      "pixels_with_surface": round(hit, 4)}))
    worker.terminate()
    mesh.dispose()
    ctx.close()


if __name__ == "__main__":
    main()
