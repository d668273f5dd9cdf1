"""-m gpu: the visibility-culled sort of a DYNAMIC-mode sorter bound to a dynamic mesh (csrc/sorter.hip: k_minmax_count<true>,
k_cull_front<MAP, true>, and k_depth_key over the compacted list) held to the sort oracle list for list, bit for bit.

The scene, the layouts of the scenes over the list, the patterns and the rig are dyn_vis_cases.py's (the mask patterns and the
sizes are vis_front_cases'; T = 2 x the device's CUs); test_dyn_vis_ref.py proves on the CPU that the case list catches a key taken
with the static rule, with the wrong scene's row, without w, with a constant w, with the scene index of the output slot, and min /
max taken over the survivors.  Every comparison (vis_front_cases.Rig.run) checks the sorted list against the oracle's dynamic
sort restricted to what the raster oracle calls visible, stats.result_count, the keep bits, key_min / key_max over ALL list
positions, visible_splats of the following draw and - where a frame is drawn - the frame against the unculled dynamic sort's.
The forced front ends run in children (tools/dyn_vis_child.py): the switch is read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dyn_vis_cases as dyn
import vis_front_cases as cases
from gaussiansplats3d_amd import Context, create_sort_worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_LABELS = ("1", "3", "33", "65", "4097")
_RIGS = {}


@pytest.fixture(scope="module")
def contexts():
    c = {"default": Context(0), "single": Context(0, single_stream=True)}
    yield c
    for rig in _RIGS.values():
        rig.close()
    _RIGS.clear()
    for v in c.values():
        v.close()


def rig_of(contexts, label, context="default", **kw):
    """One mesh and one sorter per (size, path), kept while the tests stay at that size."""
    key = (label, context, tuple(sorted(kw.items())))
    if key not in _RIGS:
        for k in [k for k in _RIGS if k[0] != label]:
            _RIGS.pop(k).close()
        T = cases.device_T()
        _RIGS[key] = dyn.DynRig(contexts[context], cases.sizes(T)[label], T, **kw)
    return _RIGS[key]


def settle(rig, bad):
    assert rig.comparisons > 0
    rig.comparisons, rig.survivors = 0, []
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("mode", dyn.MODES)
@pytest.mark.parametrize("layout", dyn.LAYOUTS)
@pytest.mark.parametrize("label", SMALL_LABELS)
def test_every_pattern_small(contexts, label, layout, mode):
    """Every pattern, both layouts of the scenes, integer centres at 16 bits and float centres at 20; every comparison draws the
    unculled dynamic sort's frame too."""
    rig = rig_of(contexts, label, layout=layout, mode=mode)
    settle(rig, cases.run_patterns(rig, cases.pattern_names(rig.n, rig.T), frame=True))


@pytest.mark.parametrize("layout,mode", list(zip(dyn.LAYOUTS, dyn.MODES)) + [("random", "int")])
@pytest.mark.parametrize("label", ["T*2048+1", "T*4096+1"])
def test_second_and_third_turn(contexts, label, layout, mode):
    """The streaming front end's second turn and its third (s_turn reused): everything, a random 30 %, the single survivors on a
    turn edge and on a chunk edge, nothing."""
    rig = rig_of(contexts, label, layout=layout, mode=mode)
    assert set(dyn.BIG_PATTERNS) <= set(cases.pattern_names(rig.n, rig.T))
    settle(rig, cases.run_patterns(rig, dyn.BIG_PATTERNS))


@pytest.mark.parametrize("layout,mode", list(zip(dyn.LAYOUTS, dyn.MODES)))
def test_compact_second_iteration(contexts, layout, mode):
    """2T*4096+1 splats: k_mask_compact's second iteration and the derive pieces' second round; no frame."""
    rig = rig_of(contexts, "2T*4096+1", layout=layout, mode=mode)
    bad = cases.run_patterns(rig, dyn.HUGE_PATTERNS, frame=False)
    bad += rig.run(cases.pattern("rand30", rig.n, rig.T), strip=cases.STRIP, frame=False, label="rand30")     # (the compact front end)
    settle(rig, bad)


@pytest.mark.parametrize("path", ["keep_order", "single", "strips_short_lifecycle", "odd_w"])
@pytest.mark.parametrize("label", dyn.PATH_LABELS)
def test_paths(contexts, label, path):
    """keep_order: a GS_MESH_KEEP_ORDER mesh has no position map - k_cull_front<false, true>, never the lazy mask - and its storage
    blocks are the list's (some without a survivor, some with a part of theirs).  single: a single-stream context.
    strips_short_lifecycle: the centre strip and a strip the column never reaches (the compact front end: k_minmax_count<true>, then
    k_depth_key over the compacted list), a list of n - 37 positions, and vis_front_cases.run_lifecycle.  odd_w: a tenth of the
    sorter's centres carry a w other than 1000 / 1.0."""
    if path == "keep_order":
        rig = rig_of(contexts, label, keep_order=True)
        assert np.array_equal(rig.storage, np.arange(rig.n))
        dead, partial = rig.block_census(cases.pattern("rand30", rig.n, rig.T) & rig.drawn)
        assert dead > 0 and partial > 0
        bad = cases.run_patterns(rig, ["all", "rand30", "mod5", "none"]) + dyn.run_paths(rig)
    elif path == "single":
        rig = rig_of(contexts, label, "single", layout="random")
        bad = cases.run_patterns(rig, ["all", "rand30", "mod5", "none"]) + dyn.run_paths(rig)
    elif path == "odd_w":
        bad = []
        for mode in dyn.MODES:
            rig = rig_of(contexts, label, layout="random", mode=mode, odd_w=True)
            bad += cases.run_patterns(rig, ["all", "rand30"]) + cases.run_strips(rig, ["rand30"])
    else:
        bad = []
        for mode in dyn.MODES:
            rig = rig_of(contexts, label, mode=mode)
            bad += dyn.run_paths(rig)
    settle(rig, bad)


def test_new_transforms_between_two_sorts(contexts):
    """set_scenes + new transforms in the sort message between two sorts of the same sorter and mesh: the second list, min / max
    and mask follow the new transforms (no stale rows in the sorter), and the expectation really moved."""
    rig = rig_of(contexts, "4097", layout="random")
    P = cases.pattern("rand30", rig.n, rig.T)
    bad = rig.run(P, label="before")
    first = rig.expected(rig.n)
    rig.set_transforms(1)
    second = rig.expected(rig.n)
    assert tuple(first[1]) != tuple(second[1]) and not np.array_equal(first[0], second[0])
    bad += rig.run(P, label="after") + rig.run(P, strip=cases.STRIP, label="after, strip")
    rig.set_transforms(0)
    bad += rig.run(P, label="back")
    settle(rig, bad)


def test_what_stays_refused(contexts):
    """Each with its message: the frustum cull on a dynamic sorter; a gathered list whose length lives on the device; a partial
    sort and precomputed distances under the cull."""
    ctx = contexts["default"]
    rig = rig_of(contexts, "4097")
    w, n = rig.worker, rig.n
    w.set_visibility_cull(True)
    rig.mesh.project(None)
    sort = {"modelViewProj": rig.mvp, "splatRenderCount": n, "splatSortCount": n}
    with pytest.raises(RuntimeError, match="full sort"):
        w.post_message({"sort": dict(sort, splatSortCount=n // 2)})
    with pytest.raises(RuntimeError, match="full sort.*without precomputed distances"):
        w.post_message({"sort": dict(sort, usePrecomputedDistances=True, precomputedDistances=np.zeros(n, np.int32))})
    settle(rig, rig.run(cases.pattern("rand30", n, rig.T), label="after the refusals"))
    d = create_sort_worker(ctx, 1000, dynamic_mode=True)
    try:
        with pytest.raises(RuntimeError, match="frustum cull is not available to a dynamic-mode sorter"):
            d.set_frustum_cull(True)
        d.set_visibility_cull(True)                        # (no longer refused)
        d.set_visibility_cull(False)
    finally:
        d.terminate()
    # a device-length gathered list: the asynchronous gather of a tree leaves the length on the device
    from gaussiansplats3d_amd import SplatTree
    import helpers
    scene = helpers.small_scene(3000, 0, seed=3)
    g = create_sort_worker(ctx, scene.count, dynamic_mode=True)
    tree = SplatTree(ctx, max_depth=5, max_centers_per_node=64).process_splat_mesh(scene.centers)
    try:
        from gaussiansplats3d_amd import util
        g.post_message({"centers": util.integer_centers(scene.centers), "sceneIndexes": np.zeros(scene.count, np.uint32),
                        "range": {"from": 0, "to": scene.count - 1, "count": scene.count}})
        tree.gather_scene_nodes_for_sort(rig.cam, sort_worker=g, to_host=False, asynchronous=True)
        with pytest.raises(RuntimeError, match="length lives on the device"):
            g.sort_gathered(rig.mvp)
    finally:
        tree.dispose()
        g.terminate()


@pytest.mark.parametrize("label", dyn.PATH_LABELS)
@pytest.mark.parametrize("front", ["stream", "compact"])
def test_forced_front_ends(front, label):
    """GSPLAT_VIS_FRONT = stream | compact forces a front end for a dynamic sorter as for a static one: every pattern of the size's
    short list, the strips and the lifecycle, both layouts, in a child process per setting."""
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "tools", "dyn_vis_child.py"), label],
                       text=True, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, GSPLAT_VIS_FRONT=front))
    tail = [l for l in p.stdout.splitlines() if l.startswith(("FAIL", "dyn_vis"))]
    print(tail[-1] if tail else p.stdout[-500:])
    assert p.returncode == 0 and tail and " 0 failures" in tail[-1] and f"front={front}" in tail[-1], "\n".join(tail[-12:]) or p.stdout[-2000:]
