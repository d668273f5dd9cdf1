"""Times a SplatRenderMode.TwoD draw of a surfel stand-in: the capture-like C3S scene (flat splats on surfaces) with every
covariance replaced by the surfel it describes - its two largest axes as scale x / y, its eigenvectors as the rotation - at the
bench's resolution.  A first measurement for DESIGN 8.17, information and not a gate.

    python tools/surfel_time.py [--config C3S] [--splats N] [--repeat 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surfels_of(cov6):
    """covariance (m00, m01, m02, m11, m12, m22) -> (scales [n,3] with the smallest axis last, rotations [n,4] x, y, z, w with w >= 0)."""
    n = cov6.shape[0]
    m = np.empty((n, 3, 3), np.float64)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2] = (cov6[:, k] for k in range(6))
    m[:, 1, 0], m[:, 2, 0], m[:, 2, 1] = m[:, 0, 1], m[:, 0, 2], m[:, 1, 2]
    val, vec = np.linalg.eigh(m)                               # ascending: the normal first
    val, vec = val[:, ::-1], vec[:, :, ::-1].copy()
    vec[:, :, 2] *= np.sign(np.linalg.det(vec))[:, None]       # a proper rotation
    r = vec
    w = np.sqrt(np.maximum(0.0, 1.0 + r[:, 0, 0] + r[:, 1, 1] + r[:, 2, 2])) / 2.0
    small = w < 1e-3                                           # (half-turns: rebuilt from the largest diagonal term would be exact;
    w = np.where(small, 1e-3, w)                               #  for a timing stand-in a clamped w is enough)
    q = np.stack([(r[:, 2, 1] - r[:, 1, 2]) / (4 * w), (r[:, 0, 2] - r[:, 2, 0]) / (4 * w), (r[:, 1, 0] - r[:, 0, 1]) / (4 * w), w], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.sqrt(np.maximum(val, 0.0)).astype(np.float32), q.astype(np.float32)


def main():
    from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3S")
    ap.add_argument("--splats", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    cfg = scenes.CONFIGS[args.config]
    scene = scenes.make_config_scene(args.config, args.splats or None)
    cam = camera.demo_camera(cfg["pose"], cfg["width"], cfg["height"])
    cov = scene.cov if not scene.cov_half else util.to_half_three(scene.cov).view(np.float16).astype(np.float32)
    scales, rotations = surfels_of(np.asarray(cov, np.float64))
    ctx = Context(0, single_stream=True)
    mesh = SplatMesh(ctx, scene.count, scene.sh_degree, render_mode_2d=True)
    mesh.build(scene.centers, None, scene.rgba, scene.sh if scene.sh_degree else None, scales=scales, rotations=rotations)
    worker = create_sort_worker(ctx, scene.count)
    worker.post_message({"centers": util.integer_centers(scene.centers), "range": {"from": 0, "to": scene.count - 1, "count": scene.count}})
    mesh.set_camera(cam)
    rows = []
    for _ in range(3 + args.repeat):                           # (the list-bin size and the bin order settle over the first draws)
        worker.sort_on_device(cam.sort_mvp(), scene.count)
        mesh.use_sorter_result(worker, scene.count)
        _, st = mesh.render(to_host=False)
        rows.append((st.device_ms, st.project_ms, st.bin_ms, st.tile_sort_ms, st.blend_ms))
    med = np.median(np.array(rows[3:]), axis=0)
    print(json.dumps({"config": args.config, "splats": scene.count, "width": cam.width, "height": cam.height, "draws": args.repeat,
                      "visible_splats": int(st.visible_splats), "tile_entries": int(st.tile_entries), "splats_walked": int(st.splats_walked),
                      "draw_ms": round(float(med[0]), 4), "project_ms": round(float(med[1]), 4), "bin_ms": round(float(med[2]), 4),
                      "tile_sort_ms": round(float(med[3]), 4), "blend_ms": round(float(med[4]), 4)}))
    worker.terminate()
    mesh.dispose()
    ctx.close()


if __name__ == "__main__":
    main()
