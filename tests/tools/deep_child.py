"""Child process of tests/test_gpu_deep_edges.py for the switches of the chunked composite that are read once per process:
GSPLAT_POOL_SLOTS (the per-bin kernel's pool of chunk partials) and GSPLAT_DEEP_MIN / GSPLAT_DEEP_FACTOR (which bins the deep pass
takes).  Draws the named cases of tests/deep_cases.py and holds every frame to the host model (tests/deep_ref.py) from the draw's
own intermediates.

usage: [GSPLAT_POOL_SLOTS=2] python tests/tools/deep_child.py pool CASE[,CASE..]
       [GSPLAT_DEEP_MIN=256 GSPLAT_DEEP_FACTOR=1] python tests/tools/deep_child.py deep CASE[,CASE..]
       -> the last line is one JSON line: a list of one record per case"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import deep_cases as cases  # noqa: E402
from gaussiansplats3d_amd import Context  # noqa: E402


def pool(rig, c):
    """The deep pass off and the pool too small: flagged, and still the composite - with the stop rule's term for ONE long chunk."""
    rig.mesh.set_deep_pass(False)
    frame, st = rig.draw()
    info = rig.mesh.deep_pass_info()
    _, Q = rig.quads()
    bad, worst, tol = cases.check_frame(frame, Q, c.w, chunks=1, what=f"{c.name} pool")
    return {"case": c.name, "pool_exhausted": bool(info["pool_exhausted"]), "flags": int(st.flags), "closed": info["chunks_closed_by_bins"],
            "bad": bad[:4], "worst": worst, "tolerance": tol}


def deep(rig, c):
    """The deep pass on a bin whose quadrants are one or two chunks deep: the same checks as with the pass on by default."""
    rig.mesh.set_deep_pass(False)
    plain, _ = rig.draw()
    _, Q = rig.quads()
    pairs_off = rig.pairs()
    sched = rig.mesh.blend_schedule()
    rig.mesh.set_deep_pass(True)
    frames = [rig.draw()[0] for _ in range(3)]
    info = rig.mesh.deep_pass_info()
    bins = {(int(b) % ((c.w + 31) // 32), int(b) // ((c.w + 31) // 32)) for b in info["bins"]}
    want = cases.expected_members(pairs_off, c, sched["deep_min"], sched["deep_factor"])
    bad, worst, tol = cases.check_frame(frames[-1], Q, c.w, what=f"{c.name} deep")
    bad += cases.check_pairs(pairs_off, Q, what="deep pass off")
    bad += cases.check_pairs(rig.pairs(), Q, bins, what="deep pass on")
    return {"case": c.name, "deep_min": sched["deep_min"], "deep_factor": sched["deep_factor"], "bins": sorted(bins), "want": sorted(want),
            "equal": [bool(np.array_equal(f, plain)) for f in frames], "closed": info["chunks_closed_by_bins"], "bad": bad[:4],
            "worst": worst, "tolerance": tol}


def main():
    what, names = sys.argv[1], sys.argv[2].split(",")
    ctx = Context(0)
    out = []
    for name in names:
        c = cases.case(name)
        rig = cases.Rig(ctx, c)
        out.append({"pool": pool, "deep": deep}[what](rig, c))
        rig.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
