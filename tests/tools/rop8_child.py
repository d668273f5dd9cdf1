"""Child process of tests/test_gpu_rop8_edges.py for 64-px list bins ($GSPLAT_LIST_SHIFT, read once per process): draws the named
cases of tests/rop8_cases.py in both shapes of the ROP8 mode and holds every frame to the interval model (tests/rop8_ref.py) from
the draw's own intermediates.

usage: GSPLAT_LIST_SHIFT=2 python tests/tools/rop8_child.py CASE[,CASE..]
       -> the last line is one JSON line: a list of one record per (case, mode)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rop8_cases as cases  # noqa: E402
import rop8_ref as rr  # noqa: E402
from gaussiansplats3d_amd import Context  # noqa: E402


def main():
    names = sys.argv[1].split(",")
    ctx = Context(0)
    out = []
    for name in names:
        c = cases.case(name)
        rig = cases.Rig(ctx, c)
        for mode in (rr.FULL, rr.BOUNDED):
            rig.mesh.set_draw_mode(rop8=True, full=mode == rr.FULL)
            frame, _ = rig.draw()
            d = rig.draw_of()
            M = rr.models_of(d, mode)
            bad, share, widest = rr.check_frame(frame, M, what=f"{name} {mode}")
            bad += rr.check_integers(rig.stats(), M, what=f"{name} {mode}")
            Mc = rr.models_of(cases.cpu_draw(c), mode)
            cpu = sum(int(m.pinned().sum()) for m in Mc.values()) / max(sum(m.lo.size for m in Mc.values()), 1)
            again = [bool(np.array_equal(rig.draw()[0], frame)) for _ in range(2)]
            lists = sorted({rr.deep_ref.list_of(d, *b) for b in c.targets})
            out.append({"case": name, "mode": mode, "list_bin_px": int(rig.mesh.last_stats().list_bin_px), "lists": lists,
                        "S": {f"{k}": m.S for k, m in M.items() if k[:2] in c.targets}, "bad": bad[:4], "pinned": share,
                        "pinned_cpu": cpu, "widest": widest, "equal": again})
        rig.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
