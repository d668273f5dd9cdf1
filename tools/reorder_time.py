"""What a progressive load's storage layout costs per frame, and what folding it costs once (information, not a
gate).  The C3 stand-in (5.8 M splats, SH-2, 1920 x 1080, the fixed demo pose) with its rows shuffled by a seeded permutation -
a trainer writes its rows in no spatial order - reaches three meshes:
  pieces   in uploads of 1 057 splats (one 262 144-byte section of 248-byte INRIA rows): about 5 500 Morton runs
  folded   the same uploads, then SplatMesh.reorder(): one run
  one      one upload: one run
Per layout: the median time of a frame (sort on the device + draw into a device buffer; a host clock around a window of frames
that ends in a device synchronise), k_project's time per launch from gs_mesh_kernel_time, visible_splats and the block-test mode
of debug read 6, and the CRC-32 of the frame.  The three layouts take turns, window by window, after a warm-up of each; the
spread over the windows is printed beside every median.  `folded` and `one` hold the same layout (tests/test_gpu_mesh_reorder.py),
so their CRC, visible_splats and block-test mode are asserted equal and their times differ by the run-to-run spread only.
python tools/reorder_time.py [--splats N] [--piece N] [--rounds K] [--frames K] [--build-order a,b,c] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util  # noqa: E402
from gaussiansplats3d_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (rehearsals)")
    ap.add_argument("--piece", type=int, default=1057)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per layout")
    ap.add_argument("--frames", type=int, default=1000, help="frames per window (a window of a fraction of a second measures the scheduler)")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--build-order", default="pieces,folded,one", help="the order in which the three meshes are created (their allocations)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    os.environ.setdefault("GSPLAT_KERNEL_SAMPLE", "4")     # the live k_project clock samples every 4th launch
    cfg = scenes.CONFIGS["C3"]
    scene = scenes.make_config_scene("C3", args.splats or None)
    n, W, H = scene.count, cfg["width"], cfg["height"]
    rows = np.random.default_rng(args.seed).permutation(n)          # the trainer's order
    data = (scene.centers[rows], scene.cov[rows], scene.rgba[rows], scene.sh[rows])
    cam = camera.demo_camera(cfg["pose"], W, H)
    mvp = cam.sort_mvp()
    ints = util.integer_centers(data[0])
    ctx = Context(0)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")

    def rig(pieces):
        mesh = SplatMesh(ctx, n, scene.sh_degree, scene.cov_half)
        step = args.piece if pieces else n
        t0 = time.perf_counter()
        for at in range(0, n, step):
            mesh.build(*(a[at:at + step] for a in data), start=at)
        upload_ms = (time.perf_counter() - t0) * 1e3
        mesh.set_camera(cam)
        worker = create_sort_worker(ctx, n)
        worker.post_message({"centers": ints, "range": {"from": 0, "to": n - 1, "count": n}})
        return {"mesh": mesh, "worker": worker, "upload_ms": upload_ms, "uploads": (n + step - 1) // step, "windows": [], "project": []}

    rigs = {name: rig(name != "one") for name in args.build_order.split(",")}
    assert sorted(rigs) == ["folded", "one", "pieces"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rigs["folded"]["mesh"].reorder()                        # (waits for the device before it returns)
    reorder_ms = (time.perf_counter() - t0) * 1e3

    def frame(r):
        r["worker"].sort_on_device(mvp, n)
        r["mesh"].use_sorter_result(r["worker"], n)
        r["mesh"].render(out_device_ptr=out.data_ptr(), to_host=False, want_stats=False)

    for r in rigs.values():                                 # warm-up: code objects, the entry buffers' growth, the list-bin size
        for _ in range(10):
            frame(r)
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in rigs.values():
            torch.cuda.synchronize()
            r["mesh"].kernel_time(0, reset=True)
            t0 = time.perf_counter()
            for _ in range(args.frames):
                frame(r)
            torch.cuda.synchronize()
            r["windows"].append((time.perf_counter() - t0) * 1e3 / args.frames)
            ms, launches = r["mesh"].kernel_time(0, reset=True)
            r["project"].append(ms / max(launches, 1))

    spread = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}   # noqa: E731
    row = {"scene": "C3 stand-in, rows shuffled by a seeded permutation (a trainer's order)", "splats": n, "width": W, "height": H,
           "piece": args.piece, "rounds": args.rounds, "frames_per_round": args.frames, "build_order": args.build_order, "reorder_ms": round(reorder_ms, 3), "layouts": {}}
    for name, r in rigs.items():
        frame(r)
        torch.cuda.synchronize()
        word = np.zeros(3, np.uint32)
        L.check(r["mesh"].lib.gs_mesh_debug_read(r["mesh"].handle, 6, word.ctypes.data, 3))
        pixels, _ = r["mesh"].render(want_stats=False)      # the fp32 frame on the host
        row["layouts"][name] = {"uploads": r["uploads"], "upload_ms": round(r["upload_ms"], 1), "frame_ms": spread(r["windows"]),
                                "k_project_ms": spread(r["project"]), "visible_splats": int(word[0]), "projected_splats": int(word[1]),
                                "block_test_mode": int(word[2]), "crc32": "%08x" % zlib.crc32(pixels.tobytes())}
    b, c = row["layouts"]["folded"], row["layouts"]["one"]
    row["frame_ms_pieces_over_one"] = round(row["layouts"]["pieces"]["frame_ms"]["median"] / c["frame_ms"]["median"], 4)
    row["k_project_ms_pieces_over_one"] = round(row["layouts"]["pieces"]["k_project_ms"]["median"] / c["k_project_ms"]["median"], 4)
    line = json.dumps(row)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for r in rigs.values():
        r["worker"].terminate()
        r["mesh"].dispose()
    ctx.close()
    same = all(b[k] == c[k] for k in ("crc32", "visible_splats", "block_test_mode"))
    assert same, "folded and one upload hold the same layout: CRC, visible_splats and block-test mode must agree"


if __name__ == "__main__":
    main()
