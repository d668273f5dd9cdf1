"""The dynamic-mode cases of tests/test_gpu_dyn_vis.py in a process of their own, for the switch that is read once per process:
GSPLAT_VIS_FRONT=stream|compact forces one front end of the visibility-culled sort, for a dynamic-mode sorter as for a static one.
Per named size (vis_front_cases.sizes) and layout of the scenes over the list (dyn_vis_cases.LAYOUTS; integer centres for `runs`,
float centres for `random`): the patterns the size's in-process test runs, the strips, a short list and the mask lifecycle.

usage: [GSPLAT_VIS_FRONT=..] python tests/tools/dyn_vis_child.py SIZE[,SIZE..]
       -> "dyn_vis: N comparisons, F failures front=... survivors min..max", exit status 1 on failure"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dyn_vis_cases as dyn
import vis_front_cases as cases
from gaussiansplats3d_amd import Context

labels = sys.argv[1].split(",")
T = cases.device_T()
sizes = cases.sizes(T)
comparisons, failures, kept = 0, [], []
ctx = Context(0)
for label in labels:
    n = sizes[label]
    for layout, mode in zip(dyn.LAYOUTS, dyn.MODES):
        rig = dyn.DynRig(ctx, n, T, layout=layout, mode=mode)
        names = cases.pattern_names(n, T) if n <= 4097 else dyn.BIG_PATTERNS
        bad = cases.run_patterns(rig, names) + dyn.run_paths(rig)
        failures += [f"{label} {layout} {mode} {b}" for b in bad]
        comparisons += rig.comparisons
        kept += rig.survivors
        rig.close()
ctx.close()
for f in failures[:40]:
    print("FAIL " + f)
print(f"dyn_vis: {comparisons} comparisons, {len(failures)} failures front={os.environ.get('GSPLAT_VIS_FRONT', 'default')} "
      f"survivors {min(kept)}..{max(kept)}")
sys.exit(1 if failures else 0)
