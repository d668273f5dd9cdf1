"""What uploads and asynchronous frames launch, library against library (the upload's host plan, csrc/upload_plan.cpp, and the two
sets of vertex-stage outputs as gs_mesh::sets must launch what the code before them launched).

usage: GSPLAT_HIP_LIB=lib.so rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/upload_plan_trace.py run
           the five uploads of tests/test_gpu_upload_plan.py (a call cut four times, gaps, a re-upload inside a merged range) into
           a Morton mesh and a GS_MESH_KEEP_ORDER mesh, then frames on a context with streams of its own: gs_mesh_project and
           gs_mesh_render alternating over two cameras, drawn from a bound sorter's visibility-culled result and from host
           indexes; prints one CRC-32 per frame read back; one process per library
       python tools/upload_plan_trace.py cmp A_kernel_trace.csv B_kernel_trace.csv
           the (kernel, grid, workgroup) lines in start order - or, where kernels of different streams started in another order,
           per queue: "identical (N launches)" or the first difference, status 1
       python tools/upload_plan_trace.py hostcall lib_a.so lib_b.so ... [--calls 3000] [--rounds 3]
           per library, interleaved in ONE process: the host's time for an asynchronous gs_mesh_render enqueue (a host clock around
           `calls` calls that end in one synchronise) and the wall time of the first upload of the C3 scene into a fresh mesh"""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

W, H = 320, 200


def cameras():
    from gaussiansplats3d_amd import camera
    return [camera.PerspectiveCamera(W, H, pos, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)) for pos in ((0.0, 0.0, 6.0), (4.0, 1.0, 5.0))]


def run():
    import test_gpu_upload_plan as t
    from gaussiansplats3d_amd import Context, SplatMesh, create_sort_worker, util
    ctx = Context(0)
    crcs = []
    for keep_order in (False, True):
        mesh = SplatMesh(ctx, t.N, 0, keep_order=keep_order)
        centres = np.zeros((t.N, 3), np.float32)
        for k, (a, b) in enumerate(t.STEPS):
            c, cov, rgba, _ = t.step_data(k)
            if k == 4:
                c = centres[a:b].copy()
                c[:, 0] = np.float32(-200.0) - c[:, 0]
            mesh.build(c, cov, rgba, None, start=a)
            centres[a:b] = c
        w = create_sort_worker(ctx, t.N)
        w.post_message({"centers": util.integer_centers(np.nan_to_num(centres)), "range": {"from": 0, "to": t.N - 1, "count": t.N}})
        mesh.use_sorter_result(w, t.N)
        w.set_visibility_cull(True)
        cams = cameras()
        for frame in range(12):                            # project -> sort -> render, the camera alternating: the sets flip every frame
            cam = cams[frame % 2]
            mesh.set_camera(cam)
            mesh.project()
            w.sort_on_device(cam.sort_mvp(), t.N)
            img, _ = mesh.render(to_host=frame >= 8, want_stats=False)
            if img is not None:
                crcs.append(zlib.crc32(img.tobytes()))
        w.set_visibility_cull(False)
        mesh.update_render_indexes(np.arange(t.N, dtype=np.uint32), t.N)
        for frame in range(6):                             # host indexes; every third frame without a gs_mesh_project of its own
            mesh.set_camera(cams[frame % 2])
            if frame % 3:
                mesh.project()
            img, _ = mesh.render(to_host=frame >= 3, want_stats=False)
            if img is not None:
                crcs.append(zlib.crc32(img.tobytes()))
        ctx.synchronize()
        w.terminate()
        mesh.dispose()
    ctx.close()
    print("upload_plan_trace: frame crcs " + " ".join("%08x" % c for c in crcs) + f" | library {os.environ.get('GSPLAT_HIP_LIB', 'of the tree')}")


def cmp(a, b):
    import csv
    from sort_plan_trace import launches

    def per_queue(path):
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        queues = {}
        for r in rows:
            queues.setdefault(r["Queue_Id"], []).append((r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])))
        return sorted(tuple(q) for q in queues.values())
    la, lb = launches(a), launches(b)
    if la == lb:
        print(f"identical ({len(la)} launches, {len(set(l[0] for l in la))} kernels, in start order)")
        return 0
    qa, qb = per_queue(a), per_queue(b)
    if qa == qb:
        print(f"identical per queue ({len(la)} launches, {len(set(l[0] for l in la))} kernels, {len(qa)} queues; kernels of different queues started in another order)")
        return 0
    if sorted(la) == sorted(lb):
        print(f"the same {len(la)} launches, distributed over the queues differently")
        return 1
    for k, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"launch {k} differs:\n  {x}\n  {y}")
            break
    print(f"{len(la)} launches against {len(lb)}")
    return 1


def hostcall(libs, calls, rounds):
    from ab_libs import use_library
    from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util
    cfg = scenes.CONFIGS["C3"]
    scene = scenes.make_config_scene("C3")
    cam = camera.demo_camera(cfg["pose"], cfg["width"], cfg["height"])
    N = scene.count
    ci = util.integer_centers(scene.centers)
    for rnd in range(rounds):
        for lib in libs:
            use_library(lib)
            ctx = Context(0)
            w = create_sort_worker(ctx, N)
            w.post_message({"centers": ci, "range": {"from": 0, "to": N - 1, "count": N}})
            ctx.synchronize()
            mesh = SplatMesh(ctx, N, scene.sh_degree, scene.cov_half)
            t0 = time.perf_counter()
            mesh.build(scene.centers, scene.cov, scene.rgba, scene.sh if scene.sh_degree else None)
            ctx.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            mesh.set_camera(cam)
            mesh.use_sorter_result(w, N)
            w.sort_on_device(cam.sort_mvp(), N)
            for _ in range(3):
                mesh.render(to_host=False, want_stats=True)
            render, handle, pc, sorter = mesh.lib.gs_mesh_render, mesh.handle, mesh._cam, w.handle     # (the bare entry point)
            import ctypes
            camp = ctypes.byref(pc)
            per_call, with_sync = [], []
            for rep in range(3):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    render(handle, camp, None, sorter, N, None, None, None)
                t1 = time.perf_counter()
                ctx.synchronize()
                per_call.append((t1 - t0) / calls * 1e6)
                with_sync.append((time.perf_counter() - t0) / calls * 1e6)
            print(f"hostcall round {rnd} {os.path.basename(lib):<20} first upload of C3 {upload_ms:8.1f} ms | asynchronous gs_mesh_render: the calls "
                  f"median {sorted(per_call)[1]:.2f} us, min {min(per_call):.2f} us per call; with the synchronise that ends them median "
                  f"{sorted(with_sync)[1]:.2f} us ({calls} calls x 3)", flush=True)
            w.terminate()
            mesh.dispose()
            ctx.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["cmp"]:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    elif sys.argv[1:2] == ["hostcall"]:
        opt = {sys.argv[k]: int(sys.argv[k + 1]) for k in range(2, len(sys.argv) - 1) if sys.argv[k].startswith("--")}
        hostcall([a for a in sys.argv[2:] if a.endswith(".so")], opt.get("--calls", 3000), opt.get("--rounds", 3))
    else:
        print(__doc__)
