"""The front-end cases of tests/test_gpu_vis_front.py in a process of their own, for the switches that are read once per process:
GSPLAT_VIS_FRONT=stream|compact forces one front end of the visibility-culled sort, GSPLAT_NO_LAZY_MASK=1 makes gs_mesh_project
write the by-original-index mask itself (one atomicOr per survivor) instead of leaving it to the bound sorter.  Per named size
(vis_front_cases.sizes): every pattern in the first context named, the strips and the mask lifecycle in every context.

usage: [GSPLAT_VIS_FRONT=..] [GSPLAT_NO_LAZY_MASK=1] python tests/tools/vis_front_child.py SIZE[,SIZE..] [patterns,strips,lifecycle] [default,single]
       -> "vis_front: N comparisons, F failures front=... lazy=... survivors min..max", exit status 1 on failure"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vis_front_cases as cases
from gaussiansplats3d_amd import Context

labels = sys.argv[1].split(",")
what = (sys.argv[2] if len(sys.argv) > 2 else "patterns,strips,lifecycle").split(",")
contexts = (sys.argv[3] if len(sys.argv) > 3 else "default").split(",")
T = cases.device_T()
sizes = cases.sizes(T)
comparisons, failures, kept = 0, [], []
for cname in contexts:
    ctx = Context(0, single_stream=True) if cname == "single" else Context(0)
    for label in labels:
        n = sizes[label]
        rig = cases.Rig(ctx, n, T)
        tag = lambda bad, part: [f"{cname} {label} {part} {b}" for b in bad]
        if "patterns" in what and cname == contexts[0]:
            failures += tag(cases.run_patterns(rig, cases.pattern_names(n, T)), "patterns")
        if "strips" in what:
            failures += tag(cases.run_strips(rig, ["rand30", "mod5"] if n > 1 else ["all"]), "strips")
        if "lifecycle" in what and n > 1:
            failures += tag(cases.run_lifecycle(rig), "lifecycle")
        comparisons += rig.comparisons
        kept += rig.survivors
        rig.close()
    ctx.close()
for f in failures[:40]:
    print("FAIL " + f)
print(f"vis_front: {comparisons} comparisons, {len(failures)} failures front={os.environ.get('GSPLAT_VIS_FRONT', 'default')} "
      f"lazy={'off' if os.environ.get('GSPLAT_NO_LAZY_MASK') else 'on'} survivors {min(kept)}..{max(kept)}")
sys.exit(1 if failures else 0)
