"""Child process of tests/test_gpu_mesh_remove.py::test_under_poisoned_allocations_in_a_child_process: one removal compared with
its fresh mesh (and one sorter removal with its fresh sorter), every object created under whatever $GSPLAT_POISON_ALLOC the parent
set.  Prints `remove_child: ok` as its last line; a failed comparison raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gaussiansplats3d_amd import Context  # noqa: E402
from test_gpu_mesh_remove import CONFIGS, removal_case  # noqa: E402
from test_gpu_sorter_remove import sorter_case  # noqa: E402


def main():
    ctx = Context(0)
    for cfg in ("sh2_fp16", "sh2_fp32_u8"):
        edited, fresh, _ = removal_case(ctx, (300, 257, 443), [1], CONFIGS[cfg], capacity=1500)
        edited.dispose()
        fresh.dispose()
    sorter_case(ctx, integer=True, dynamic=False)
    ctx.close()
    print("remove_child: ok")


if __name__ == "__main__":
    main()
