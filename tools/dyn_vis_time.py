"""Times the visibility-culled sort of a DYNAMIC-mode sorter next to the static one, in one process on one box: the bench's C3
stand-in (5.8 M splats) split into four scenes back to back with distinct rigid transforms, a full 1920 x 1080 frame and a 1/8
strip of its tile rows.  Per frame kind: the static visibility-culled sort, the dynamic visibility-culled sort and the dynamic
unculled sort - gs_sort_stats.device_ms, the stage-events clock (GS_CTX_STAGE_TIMING: one event pair around every sort).
By bytes the static streaming front end reads 16 B per position (three centre planes and the payload map) and the dynamic one 24 B
(w and the scene index on top): the expectation to check is 1.5 x the static kernel's time.  Information, not a gate: DESIGN 8.2a
records the measured table (profiles/dyn_vis_time.txt: k_cull_front 34.3 -> 43.5 us, 1.27 x; k_minmax_count 17.4 -> 26.2 us).
The dynamic culled FULL-frame sort is slower than the dynamic unculled one (0.136 against 0.078 ms there): a full frame's cull pays
only through the draw behind it.  The strip (0.076 ms, 265 k of 5.8 M splats kept) is what the feature exists for.

The front-end kernels' own times come from a second step: the same sorts in child processes under `rocprofv3 --kernel-trace
--stats`, one child per group (static, dynamic culled, dynamic unculled) so that every kernel name belongs to one frame kind - a
full frame takes the streaming front end (k_mask_derive_count + k_cull_front), a strip the compact one (k_minmax_count +
k_mask_compact + k_depth_key over the survivors).  --no-kernels skips that step.

    python tools/dyn_vis_time.py [--config C3] [--repeat 20] [--no-kernels]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = ("static_culled", "dynamic_culled", "dynamic_unculled")
FRONT_KERNELS = ("k_mask_derive_count", "k_mask_count", "k_cull_front", "k_minmax_count", "k_mask_compact", "k_depth_key", "k_store_scene_rows")


def rigid(axis, deg, t, about):
    """Column-major 16-vector: a turn of `deg` about `axis` through the point `about`, then the translation t."""
    a = np.deg2rad(deg)
    R = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i] = R[j, j] = np.cos(a); R[i, j] = -np.sin(a); R[j, i] = np.sin(a)
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = about - R @ about + np.asarray(t)
    return M.T.reshape(16)


def measure(config, groups, repeat):
    """{group: {frame kind: {...}}} - every group in this process."""
    from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util

    cfg = scenes.CONFIGS[config]
    scene = scenes.make_config_scene(config)
    n = scene.count
    cam = camera.demo_camera(cfg["pose"], cfg["width"], cfg["height"])
    rows = (cfg["height"] + 15) // 16
    kinds = {"full": None, "strip_1_8": (rows * 4 // 8, rows * 5 // 8)}
    mid = scene.centers.mean(axis=0, dtype=np.float64)
    transforms = [rigid(1, 3.0, (0.05, 0.0, -0.04), mid), rigid(0, -2.0, (-0.03, 0.06, 0.0), mid), rigid(2, 4.0, (0.0, -0.05, 0.05), mid),
                  rigid(1, -5.0, (0.04, 0.04, 0.0), mid)]
    scene_idx = np.minimum(np.arange(n, dtype=np.int64) * 4 // n, 3).astype(np.uint32)     # four scenes back to back
    tr32 = np.concatenate(transforms).astype(np.float32)
    ci = util.integer_centers(scene.centers)
    mvp = cam.sort_mvp()
    ctx = Context(0, stage_timing=True)
    out = {}
    for dynamic in (False, True):
        mine = [g for g in groups if g.startswith("dynamic" if dynamic else "static")]
        if not mine:
            continue
        mesh = SplatMesh(ctx, n, 0, dynamic_mode=dynamic)
        mesh.build(scene.centers, scene.cov, scene.rgba, scene_indexes=scene_idx if dynamic else None)
        if dynamic:
            mesh.set_scenes(transforms=transforms, camera_position=cam.position)
        mesh.set_camera(cam)
        w = create_sort_worker(ctx, n, dynamic_mode=dynamic)
        w.post_message({"centers": ci, "sceneIndexes": scene_idx, "range": {"from": 0, "to": n - 1, "count": n}})
        sort = {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n, "transforms": tr32, "keepOnDevice": True}
        w.post_message({"sort": sort})
        mesh.use_sorter_result(w, n)                          # the bind
        for g in mine:
            culled = not g.endswith("unculled")
            w.set_visibility_cull(culled)
            out[g] = {}
            for kind, strip in kinds.items():
                if not culled and strip is not None:
                    continue                                  # (the unculled sort does not know about strips)
                ms, kept = [], n
                for k in range(repeat + 3):
                    if culled:
                        mesh.project(strip)
                    w.post_message({"sort": sort})
                    st, _ = w.last_stats()                    # (waits for the sort)
                    if k >= 3:
                        ms.append(float(st.device_ms))
                    kept = int(st.result_count)
                    if culled:
                        mesh.use_sorter_result(w, n)
                        mesh.render(tile_rows=strip, to_host=False, want_stats=False)      # consumes the projection
                ms.sort()
                out[g][kind] = {"sort_ms_median": round(ms[len(ms) // 2], 4), "sort_ms_min": round(ms[0], 4), "sort_ms_max": round(ms[-1], 4),
                                "kept": kept, "kept_frac": round(kept / n, 4)}
        w.terminate()
        mesh.dispose()
    ctx.close()
    return {"config": config, "splats": n, "scenes": 4, "repeat": repeat, "clock": "gs_sort_stats.device_ms with GS_CTX_STAGE_TIMING", "sort": out}


def kernel_rows(config, group, repeat):
    """{kernel: avg us} of the front-end kernels of one group, from a child of this script under rocprofv3."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--config", config, "--repeat", str(repeat), "--groups", group, "--no-kernels"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not found:
            return {"error": p.stdout[-400:]}
        rows = {}
        for r in csv.DictReader(open(found[0])):
            name = re.sub(r"\(.*", "", r["Name"]).replace("void ", "")
            if name.startswith(FRONT_KERNELS):
                rows[name] = {"avg_us": round(float(r["AverageNs"]) / 1e3, 2), "calls": int(r["Calls"])}
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--groups", default=",".join(GROUPS))
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    groups = args.groups.split(",")
    if args.no_kernels:
        print(json.dumps(measure(args.config, groups, args.repeat)))
        return
    # the parent never opens the device: the measurement and the profiled runs are children of their own
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", args.config, "--repeat", str(args.repeat), "--groups",
                        args.groups, "--no-kernels"], stdout=subprocess.PIPE, text=True, timeout=900)
    print(p.stdout.strip())
    if p.returncode != 0:
        raise SystemExit(p.returncode)
    for g in groups:
        print(json.dumps({"kernels_under_rocprofv3": g, "rows": kernel_rows(args.config, g, max(3, args.repeat // 4))}))


if __name__ == "__main__":
    main()
