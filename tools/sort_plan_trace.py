"""What a depth sort launches, library against library (the sort's host plan, csrc/sort_plan.cpp, must launch what the code before
it launched).

usage: GSPLAT_HIP_LIB=lib.so rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sort_plan_trace.py run
           one sort per front-end kind and pass-chain shape (the kinds of tests/test_gpu_sort_plan.py, 4097 and 24577 splats) on a
           single-stream context, so that the trace's order is the order of the launches; one process per library
       python tools/sort_plan_trace.py cmp A_kernel_trace.csv B_kernel_trace.csv [--print]
           the sequences of (kernel, grid, workgroup) in start order: "identical (N launches)" or the first difference, status 1
       python tools/sort_plan_trace.py hostcall lib_a.so lib_b.so ... [--calls 4000] [--rounds 3]
           the host's time for one gs_sorter_sort that launches nothing (render_count = 0), per library, interleaved in ONE process"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SIZES = (4097, 3 * 4096 * 2 + 1)


def run():
    import helpers
    import kat_cases
    import known_range_cases as kr
    import vis_front_cases as vf
    from gaussiansplats3d_amd import Context, SplatTree, camera, create_sort_worker, util
    ctx = Context(0, single_stream=True)
    sorts = 0
    for n in SIZES:
        for precision, scale in ((16, 3000.0), (16, 30000.0), (20, 3000.0)):          # known range: compact, narrow, wide
            ci = kr.gaussian_centers(n, seed=n + precision, scale=scale)
            w = create_sort_worker(ctx, n, splat_sort_distance_map_precision=precision)
            kr.upload(w, ci)
            for k in range(2):
                w.sort_on_device(kr.camera_mvp(k), n)
                sorts += 1
            w.set_frustum_cull(True)                                                   # the frustum cull: identity and index list
            w.sort_on_device(kr.camera_mvp(0), n)
            w.sort_on_device(kr.camera_mvp(0), n, indexes=np.random.default_rng(n).permutation(n).astype(np.uint32))
            sorts += 2
            w.terminate()
        for case in (dict(name="partial", sort=n // 3), dict(name="host_list", permute=True, render=n - 5, sort=n - 5),
                     dict(name="float_p20", mode="float", precision=20), dict(name="dynamic", dynamic=True), dict(name="precomputed", precomputed=True)):
            case = dict(dict(n=n, precision=16, mode="int", render=n), **case)
            case.setdefault("sort", case["render"])
            a = kat_cases.make_case(case)
            w = create_sort_worker(ctx, n, True, True, a["use_int"], a["dynamic"], a["precision"])
            w.post_message({"centers": a["centers4"], "sceneIndexes": a["scene_indexes"], "range": {"from": 0, "to": n - 1, "count": n}})
            w.post_message({"sort": {"modelViewProj": a["mvp"], "splatRenderCount": a["render_count"], "splatSortCount": a["sort_count"],
                                     "usePrecomputedDistances": a["precomputed"] is not None, "indexesToSort": a["indexes"] if case.get("permute") else None,
                                     "transforms": a["transforms"], "precomputedDistances": a["precomputed"], "keepOnDevice": True}})
            sorts += 1
            w.terminate()
        rig = vf.Rig(ctx, n, vf.device_T())                                            # the visibility cull: full frame, strip, full frame
        P = vf.pattern("rand30", n, rig.T)
        for strip in (None, vf.STRIP, None):
            assert rig.run(P, strip=strip, frame=False) == []
            sorts += 1
        rig.close()
        c = helpers.small_scene(n, 0, seed=n).centers                                  # gathered lists: fused, culled, asynchronous, partial
        cam = camera.demo_camera("garden", 640, 360)
        tree = SplatTree(ctx, 8, 200).process_splat_mesh(c)
        w = create_sort_worker(ctx, n)
        w.post_message({"centers": util.integer_centers(c), "range": {"from": 0, "to": n - 1, "count": n}})
        for cull, asynchronous in ((False, False), (True, False), (False, True), (True, True)):
            w.set_frustum_cull(cull)
            tree.gather_scene_nodes_for_sort(cam, sort_worker=w, to_host=False, asynchronous=asynchronous)
            w.sort_gathered(cam.sort_mvp(), keep_on_device=True)
            sorts += 1
        w.set_frustum_cull(False)
        r = tree.gather_scene_nodes_for_sort(cam, sort_worker=w, to_host=False)
        w.sort_gathered(cam.sort_mvp(), r["splatRenderCount"] // 2, keep_on_device=True)
        sorts += 1
        w.last_stats()                                                                 # (synchronises)
        w.terminate()
        tree.dispose()
    ctx.close()
    print(f"sort_plan_trace: {sorts} sorts, library {os.environ.get('GSPLAT_HIP_LIB', 'of the tree')}")


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")) for r in rows]


def cmp(a, b, show):
    la, lb = launches(a), launches(b)
    if show:
        for name, grid, wg in la:
            print(f"{grid[0]:>8} x {wg[0]:<5} {name[:150]}")
    for k, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"launch {k} differs:\n  {x}\n  {y}")
            return 1
    if len(la) != len(lb):
        print(f"{len(la)} launches against {len(lb)}")
        return 1
    print(f"identical ({len(la)} launches, {len(set(l[0] for l in la))} kernels)")
    return 0


def hostcall(libs, calls, rounds):
    from ab_libs import use_library
    from gaussiansplats3d_amd import Context, create_sort_worker
    import known_range_cases as kr
    n = 4097
    ci = kr.gaussian_centers(n, seed=1)
    for rnd in range(rounds):
        for lib in libs:
            use_library(lib)
            ctx = Context(0, single_stream=True)
            w = create_sort_worker(ctx, n)
            kr.upload(w, ci)
            w.sort_on_device(kr.camera_mvp(0), n)
            mvp = np.ascontiguousarray(kr.camera_mvp(0), dtype=np.float32)
            sort, handle, pm = w.lib.gs_sorter_sort, w.handle, mvp.ctypes.data       # (the bare entry point: no wrapper work in the loop)
            best = []
            for rep in range(5):
                t0 = time.perf_counter()
                for _ in range(calls):
                    sort(handle, pm, None, 0, 0, None, None, None, None)
                best.append((time.perf_counter() - t0) / calls * 1e6)
            print(f"hostcall round {rnd} {os.path.basename(lib):<20} gs_sorter_sort(render_count = 0) through ctypes: "
                  f"median {sorted(best)[2]:.3f} us, min {min(best):.3f} us per call ({calls} calls x 5)")
            w.terminate()
            ctx.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["cmp"]:
        sys.exit(cmp(sys.argv[2], sys.argv[3], "--print" in sys.argv))
    elif sys.argv[1:2] == ["hostcall"]:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        args = [a for a in sys.argv[2:] if not a.startswith("--")]
        opt = {sys.argv[k]: int(sys.argv[k + 1]) for k in range(2, len(sys.argv) - 1) if sys.argv[k].startswith("--")}
        libs = [a for a in args if a.endswith(".so")]
        hostcall(libs, opt.get("--calls", 4000), opt.get("--rounds", 3))
    else:
        print(__doc__)
