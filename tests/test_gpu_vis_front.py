"""-m gpu: the front ends of the visibility-culled sort (csrc/sorter.hip: k_mask_count, k_cull_front<MAP>, k_minmax_count,
k_mask_compact, k_mask_derive_count) held to the sort oracle list for list, bit for bit, on masks the test dictates.

The frame-equality checks of the soaks cannot see these kernels fail: the binner tests visibility again, so a spurious or
misplaced survivor changes no pixel.  Here every comparison is the whole contract (vis_front_cases.Rig.run): the sorted list is
the oracle's order restricted to the constructed mask, stats.result_count its population, the sorter's keep bits the mask,
(key_min, key_max) the oracle's over ALL list positions, and the following draw reports as many visible splats and equals the
frame of the unculled sort.  Sizes sit where the chunked kernels change behaviour (vis_front_cases.sizes; T = 2 x the device's
CUs), patterns where masks alias nibbles, words, ballots, turns and chunks (the boundary positions come from the host model,
vis_front_ref.geometry); test_vis_front_ref.py proves on the CPU that the list catches every mutation of that model.
Switches read once per process run in children (tools/vis_front_child.py).

Measured on an MI355X with two deliberately wrong builds of the library: min / max taken over the survivors in k_cull_front fails
73 of the 75 in-process tests here; s_turn left single buffered fails none - the race needs a wave to stall between the turn's
barrier and the four LDS reads right behind it while another wave finishes a whole turn, and no deterministic input arranges
that (an observation, not a proof that it cannot happen).  The model's turn_parity_reused mutation is a deterministic stand-in for
that mistake - turn t reads the counts turn t - 2 left - not the same bug, so the device tier does not hold it."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import vis_front_cases as cases
from gaussiansplats3d_amd import Context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = list(cases.sizes(512))                    # the labels do not depend on T
MIXED = ("rand30", "mod5", "w64", "w32")            # patterns that hide a part of a storage block (the input condition of the gather)
_RIGS = {}
TOTAL = {"comparisons": 0, "kept": []}


@pytest.fixture(scope="module")
def contexts():
    c = {"default": Context(0), "single": Context(0, single_stream=True)}
    yield c
    for rig in _RIGS.values():
        rig.close()
    _RIGS.clear()
    kept = TOTAL["kept"] or [0]
    print(f"\nvis_front (in process): {TOTAL['comparisons']} comparisons, survivors {min(kept)}..{max(kept)}")
    for v in c.values():
        v.close()


def rig_of(contexts, label, context="default", **kw):
    """One mesh and one sorter per (size, path), kept while the tests stay at that size."""
    key = (label, context, tuple(sorted(kw.items())))
    if key not in _RIGS:
        for k in [k for k in _RIGS if k[0] != label]:
            _RIGS.pop(k).close()
        T = cases.device_T()
        _RIGS[key] = cases.Rig(contexts[context], cases.sizes(T)[label], T, **kw)
    return _RIGS[key]


def settle(rig, bad):
    TOTAL["comparisons"] += rig.comparisons
    TOTAL["kept"] += rig.survivors
    rig.comparisons, rig.survivors = 0, []
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("third", [0, 1, 2])
@pytest.mark.parametrize("label", LABELS)
def test_every_pattern_on_the_default_path(contexts, label, third):
    """Default context, integer centres at 16 bits, Morton mesh, full frame: the lazy path (k_mask_derive_count, k_cull_front<true>).
    The scene must exercise the gather: some storage blocks without any survivor, some with a part of theirs."""
    rig = rig_of(contexts, label)
    names = cases.pattern_names(rig.n, rig.T)
    if third == 0 and rig.n >= 4095:
        for mixed in MIXED:
            dead, partial = rig.block_census(cases.pattern(mixed, rig.n, rig.T) & ~rig.scene.behind)
            assert dead > 0 and partial > 0, (mixed, dead, partial)
    settle(rig, cases.run_patterns(rig, names[third::3]))


@pytest.mark.parametrize("path", ["float", "keep_order", "single", "fewer_centres"])
@pytest.mark.parametrize("label", cases.PATH_SIZES)
def test_every_pattern_on_the_other_paths(contexts, label, path):
    """float: float centres at precision 20 (static_key_float in k_cull_front).  keep_order: a GS_MESH_KEEP_ORDER mesh has no position
    map - k_cull_front<false>, never lazy.  single: a single-stream context (one record set).  fewer_centres: the sorter has received
    n - 37 centres of a mesh of n, so the list is shorter than the projection.  The float and keep-order rigs also run the
    strips, which take the compact front end."""
    kw = {"float": {"float_centres": True}, "keep_order": {"keep_order": True}, "single": {}, "fewer_centres": {}}[path]
    n = cases.sizes(cases.device_T())[label]
    if path == "fewer_centres":
        kw = {"sorter_count": n - cases.SHORT[0]}
    rig = rig_of(contexts, label, "single" if path == "single" else "default", **kw)
    names = cases.pattern_names(rig.n, rig.T)
    if rig.n > 3_000_000:                                  # the largest size: the patterns that differ per turn, word and chunk
        names = [p for p in names if p in ("all", "none", "last", "rand30", "w64", "mod5") or p.startswith(("stream:", "lazy:turn"))]
    if path == "keep_order" and rig.n >= 4095:
        assert np.array_equal(rig.storage, np.arange(rig.n))
        for mixed in MIXED:
            dead, partial = rig.block_census(cases.pattern(mixed, rig.n, rig.T) & ~rig.scene.behind)
            assert dead > 0 and partial > 0, (mixed, dead, partial)
    bad = cases.run_patterns(rig, names)
    if path in ("float", "keep_order"):
        # a strip goes through k_minmax_count + k_mask_compact + k_depth_key: with float centres the scalar branch of
        # k_minmax_count (and its min / max over all positions), with a keep-order mesh a compaction without a position map
        bad += cases.run_strips(rig, ["rand30", "mod5"] if rig.n > 1 else ["all"])
    settle(rig, bad)


@pytest.mark.parametrize("label", cases.PATH_SIZES)
def test_strips_and_short_lists(contexts, label):
    """The centre strip keeps the full frame's mask (vertex stage atomics, compact front end), a far strip keeps nothing; lists of
    n - 37 and n - 38 positions through splatRenderCount leave set bits beyond the list in the mask."""
    rig = rig_of(contexts, label)
    bad = cases.run_strips(rig, ["all", "rand30", "mod5"])
    for d in cases.SHORT:
        if rig.n > d:
            bad += cases.run_patterns(rig, ["all", "rand30", "mod5", "last"] if rig.n > 1 else ["all"], R=rig.n - d)
    settle(rig, bad)


@pytest.mark.parametrize("context", ["default", "single"])
@pytest.mark.parametrize("label", ["4097", "2T*4096+1"])
def test_mask_lifecycle(contexts, label, context):
    """A, complement of A, A; around short lists, strips and projections nobody consumed - per context (the default one keeps two
    record sets, each with its own mask and flags)."""
    rig = rig_of(contexts, label, context)
    settle(rig, cases.run_lifecycle(rig))


def test_non_coarse_branch_of_the_derived_mask(contexts):
    """16 777 217 splats = 65537 storage blocks: k_mask_derive_count reads block_any from memory instead of its bits in LDS.  One
    pattern, SH-0, half covariances; its wall time is printed (pytest -s)."""
    t0 = time.perf_counter()
    for k in list(_RIGS):
        _RIGS.pop(k).close()
    rig = cases.Rig(contexts["default"], cases.NONCOARSE, cases.device_T(), half_cov=True)
    try:
        assert (rig.n + 255) // 256 == 65537
        bad = cases.run_patterns(rig, ["rand30"])
    finally:
        rig.close()
    print(f"\nnon-coarse case: {time.perf_counter() - t0:.1f} s, {rig.survivors[0]} survivors of {rig.n}")
    settle(rig, bad)


CHILDREN = {"stream": {"GSPLAT_VIS_FRONT": "stream"}, "compact": {"GSPLAT_VIS_FRONT": "compact"},
            "no_lazy": {"GSPLAT_NO_LAZY_MASK": "1"}, "no_lazy_compact": {"GSPLAT_NO_LAZY_MASK": "1", "GSPLAT_VIS_FRONT": "compact"}}
# (child, what it runs, context): every pattern in the default context; strips and lifecycle in the default context, and for
# the eager mask (whose set bits accumulate by atomicOr) in the single-stream context as well - one child per context
CHILD_RUNS = [(c, part, ctx) for c in CHILDREN for part, ctx in (("patterns", "default"), ("strips,lifecycle", "default"),
                                                                 ("strips,lifecycle", "single"))
              if (c, part) != ("no_lazy_compact", "patterns") and (ctx == "default" or c.startswith("no_lazy"))]


@pytest.mark.parametrize("label", cases.FORCED_SIZES)
@pytest.mark.parametrize("child,part,context", CHILD_RUNS)
def test_forced_front_ends_and_the_eager_mask(child, part, context, label):
    """Both front ends forced (after the lazy derive, and after the vertex stage's atomics) and the default choice with
    GSPLAT_NO_LAZY_MASK=1, in a child process per setting: every pattern, the strips and the lifecycle."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "vis_front_child.py"), label, part, context], text=True,
                       timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, **CHILDREN[child]))
    tail = [l for l in p.stdout.splitlines() if l.startswith(("FAIL", "vis_front"))]
    print(tail[-1] if tail else p.stdout[-500:])
    assert p.returncode == 0 and tail and " 0 failures" in tail[-1], "\n".join(tail[-12:]) or p.stdout[-2000:]
