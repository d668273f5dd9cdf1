"""Child process of tests/test_gpu_bounds.py::test_under_poisoned_allocations_in_a_child_process: gs_mesh_bounds over a mesh that is
larger than what was uploaded, created under whatever $GSPLAT_POISON_ALLOC the parent set.  Prints one JSON line of results; the
parent compares them with the host model."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import reveal_cases  # noqa: E402
from gaussiansplats3d_amd import Context, SplatMesh  # noqa: E402
from test_gpu_bounds import CENTER, cloud, mesh_of  # noqa: E402


def main():
    ctx = Context(0)
    c = cloud(700, 17)
    idx = (np.arange(700) % 2).astype(np.uint32)
    transforms = next(b for b in reveal_cases.kat()["bounds"] if b["name"] == "two_scenes")["transforms"]
    mesh = mesh_of(ctx, c, capacity=2000, uploads=[(0, 257), (257, 700)], scene_indexes=idx, dynamic_mode=True)
    rows = []
    for start, count, moved in [(0, 700, False), (0, 700, True), (200, 100, True), (257, 443, False)]:
        b = mesh.bounds(start, count, CENTER, transforms if moved else None)
        rows.append({"start": start, "count": count, "transformed": moved, "count_out": b["count"], "min": b["min"].tolist(),
                     "max": b["max"].tolist(), "max_dist_sq": float(b["max_dist_sq"]).hex()})
    mesh.dispose()
    ctx.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
