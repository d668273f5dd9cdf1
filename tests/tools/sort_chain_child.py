"""The rows of tests/sort_chain_cases.py that need a switch which is read once per process, in a process of their own: the edge
rows of integer 16, integer 20 and float 24 (child_cells) - every sort against the sort oracle, the executed inputs
(gs_sorter_debug_read, selector 5) showing the switch, the executed plan equal to the host model's and to the chain
tests/test_sort_chains.py counted on.  That holds for GSPLAT_NO_SORT_CHUNK and GSPLAT_NO_SORT_PACK, which are plan inputs.
GSPLAT_NO_LDS_ATOMIC_RANK is read by gs_context_create into a field no entry point hands out: that child's sorts are held to the
oracle and the model like the others, but that they took the ballot ranking is NOT verified here - it rests on the variable's name
(csrc/context.hip) alone.

usage: GSPLAT_NO_SORT_CHUNK=1 | GSPLAT_NO_SORT_PACK=1 | GSPLAT_NO_LDS_ATOMIC_RANK=1  python tests/tools/sort_chain_child.py SWITCH
       -> "sort_chain_child SWITCH: ok"; an exception (exit status 1) on a failure"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sort_chain_cases as cc  # noqa: E402
from gaussiansplats3d_amd import Context  # noqa: E402

switch = sys.argv[1]
assert switch in cc.SWITCHES and os.environ.get(switch), "the switch has to be set in the environment"
import torch  # noqa: E402
cus = torch.cuda.get_device_properties(0).multi_processor_count
ctx = Context(0)                                           # (GSPLAT_NO_LDS_ATOMIC_RANK is read here, the others at the first sort)
t0, sorts = time.time(), 0
for cell in cc.child_cells(switch):
    sorts += len(cc.run_cell(ctx, cell, cus, switch=switch, log=print if "-v" in sys.argv else None))
ctx.close()
print(f"sort_chain_child {switch}: ok ({sorts} sorts, {time.time() - t0:.1f} s)")
