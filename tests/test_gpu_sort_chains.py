"""-m gpu: the matrix of sort_chain_cases.py on the device.  tests/test_sort_chains.py proves (without a GPU) that these cells and
the children below reach every radix pass chain csrc/sort_plan.cpp can plan; here every sort of every cell is held to the sort
oracle bit for bit - list, keys, buckets, key_min / key_max, clamped, status - and its executed plan (gs_sorter_debug_read,
selector 5) to the host model and to the chain the proof counted on.  One worker is alive at a time."""
import os
import subprocess
import sys

import pytest

import sort_chain_cases as cc
from gaussiansplats3d_amd import Context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = cc.cells()


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(ctx, cus, cells):
    assert cells
    done = []
    for cell in cells:
        done += [(cell, *d) for d in cc.run_cell(ctx, cell, cus)]
    return done


@pytest.mark.parametrize("n", cc.SWEEP_N)
@pytest.mark.parametrize("data", ("gauss", "grid"))
@pytest.mark.parametrize("mode", ("int", "float"))
def test_precision_sweep(ctx, cus, mode, data, n):
    """Every precision of the mode (integer 10..20: the identity list twice, a partial sort, a permuted host list, both lists
    under the frustum cull; float 10..24: the full sort), on Gaussian centres and on a grid of many exactly equal keys."""
    done = _run(ctx, cus, [c for c in CELLS if c["kind"] == "sweep" and (c["mode"], c["data"], c["max_count"]) == (mode, data, n)])
    assert {c["precision"] for c, *_ in done} == set(cc.INT_PRECISIONS if mode == "int" else cc.FLOAT_PRECISIONS)


@pytest.mark.parametrize("n", cc.SWEEP_N)
def test_dynamic_and_precomputed_front_ends(ctx, cus, n):
    """Dynamic integer, precomputed integer and precomputed float sorters at precisions 10, 13, 17, 20 (float: and 24)."""
    _run(ctx, cus, [c for c in CELLS if c["kind"] == "front" and c["max_count"] == n])


@pytest.mark.parametrize("name", [c["name"] for c in CELLS if c["kind"] == "edge"])
def test_payload_width_edge(ctx, cus, name):
    """One sorter grown through set_uploaded_count to either side of the `uploaded` at which pass 0 stops packing or the passes
    stop staging chunks; at each, a host list holding uploaded - 1, plain, under the frustum cull and keyed by precomputed
    distances."""
    cell, = [c for c in CELLS if c["name"] == name]
    done = _run(ctx, cus, [cell])
    for kind in cc.EDGE_SORTS:                               # (plain, culled, precomputed: each at every step)
        assert sorted({u for _, u, sort, _ in done if sort == kind}) == [u for u, _ in cell["steps"]]


def test_float_24_clamps_where_the_oracle_does(ctx, cus):
    """The cells of float precision 24 whose farthest splat lands in bucket `range` report it (status 1, SortFrame::clamped), the
    others report nothing: both kinds exist (tests/test_sort_chains.py) and run_cell held each count to the oracle's."""
    done = _run(ctx, cus, [c for c in CELLS if c["kind"] in ("sweep", "front") and c["mode"] == "float" and c["precision"] == 24])
    assert any(k > 0 for *_, k in done) and any(k == 0 for *_, k in done)


def test_large_identity_sort_with_eight_million_equal_keys(ctx, cus):
    """uploaded = 2^23 + 1 at precision 16: the zero rows between the two real ranges take part, one bucket (one digit count of
    each pass) holds more than 2^23 elements, through the known-range front end and two chunk-staged passes."""
    cell, = [c for c in CELLS if c["kind"] == "big"]
    import sort_plan_ref as ref
    want = ref.sort_plan(cc.plan_inputs(cell, cc.BIG_U, (cc.FULL, 0, 0)))
    assert want["known_range"] and [p["chunked"] for p in want["pass"][:2]] == [1, 1] and want["val_bits"] == 24
    _run(ctx, cus, [cell])


def test_switches_read_once_per_process():
    """The packed passes through the tile kernel at 24 bits, the key + value chains with payload bit 24, and the ballot ranking:
    the edge rows of integer 16, integer 20 and float 24 in one child process per switch.  The three run at once, as the children
    of test_gpu_sort_plan.py do, so that the test stays within a few seconds: one large sorter per PROCESS is alive at a time,
    three on the device (3 x 1.2 GB at most)."""
    script = os.path.join(ROOT, "tests", "tools", "sort_chain_child.py")
    procs = [(sw, subprocess.Popen([sys.executable, script, sw], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   env=dict(os.environ, **{sw: "1"}))) for sw in cc.SWITCHES]
    failed = []
    for sw, p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            out += "\n(timed out)"
        if p.returncode != 0 or f"sort_chain_child {sw}: ok" not in out:
            failed.append(f"--- {sw} (exit status {p.returncode})\n{out[-2000:]}")
    assert not failed, "\n".join(failed)
