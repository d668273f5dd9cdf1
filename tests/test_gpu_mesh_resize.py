"""-m gpu: gs_mesh_resize held to its definition - afterwards the mesh behaves, in every output, as a fresh mesh of the new
capacity and the same flags that received the same splats by the same uploads.  Every scene is one upload (one Morton run); the
layouts put run borders inside a storage block with the end in a partial block, and on block edges.  Compared with the fresh mesh,
byte for byte (test_gpu_mesh_remove's comparison): gs_mesh_debug_read 10 / 11 / 12 over every block of the new capacity, a 64 x 64
frame from one shared host order in fp32 and both ROP8 modes, gs_mesh_surface and gs_mesh_bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gaussiansplats3d_amd import Context, GsError, camera
from gaussiansplats3d_amd import _lib as L
from test_gpu_mesh_remove import CONFIGS, LAYOUTS, frames, new_mesh, planes, same_as_fresh, scene_data, upload_runs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# capacities a mesh of 1000 uploaded splats goes through, one resize each
PAIRS = {"1000_1001": (1000, 1001),                        # same block count, a capacity that is no multiple of 4
         "1000_1025": (1000, 1025),                        # one more block
         "1024_2048": (1024, 2048),
         "1400_1000": (1400, 1000),                        # down to exactly the uploaded count
         "1400_1024": (1400, 1024),
         "1000_5000_1000": (1000, 5000, 1000)}             # there and back
# (configuration, GS_MESH_KEEP_ORDER, single-stream context = one record set)
VARIANTS = {"sh0_fp32": ("sh0_fp32", False, False), "sh2_fp16": ("sh2_fp16", False, False), "sh2_fp32_u8": ("sh2_fp32_u8", False, False),
            "keep_order": ("sh2_fp16", True, False), "single_stream": ("sh2_fp32_u8", False, True),
            "keep_order_single_stream": ("sh0_fp32", True, True)}


@pytest.fixture(scope="module")
def contexts():
    c = {False: Context(0), True: Context(0, single_stream=True)}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts[False]


def runs_of(sizes, cfg, seed=40):
    return [scene_data(n, cfg["deg"], seed + k, cfg["u8"]) for k, n in enumerate(sizes)]


def resize_case(ctx, sizes, capacities, cfg, **kw):
    """uploads the runs into a mesh of capacities[0], draws, then walks the other capacities: after every resize the mesh is
    compared with a fresh one of that capacity; returns (edited, the last fresh mesh, runs)"""
    runs = runs_of(sizes, cfg)
    edited = new_mesh(ctx, capacities[0], cfg, **kw)
    upload_runs(edited, runs)
    edited.render()                                        # (a draw before: its state must not leak into the frames after)
    fresh = None
    for capacity in capacities[1:]:
        edited.resize(capacity)
        assert edited.max_splat_count == capacity
        if fresh is not None:
            fresh.dispose()
        fresh = new_mesh(ctx, capacity, cfg, **kw)
        upload_runs(fresh, runs)
        same_as_fresh(edited, fresh, capacity)
    return edited, fresh, runs


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
@pytest.mark.parametrize("pair", list(PAIRS), ids=list(PAIRS))
@pytest.mark.parametrize("sizes", LAYOUTS, ids=["x".join(map(str, s)) for s in LAYOUTS])
def test_a_resize_leaves_a_fresh_mesh(contexts, sizes, pair, variant):
    cfg, keep_order, single = VARIANTS[variant]
    kw = dict(keep_order=True) if keep_order else {}
    edited, fresh, _ = resize_case(contexts[single], sizes, PAIRS[pair], CONFIGS[cfg], **kw)
    edited.dispose()
    fresh.dispose()


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
def test_an_empty_mesh(contexts, variant):
    cfg, keep_order, single = VARIANTS[variant]
    kw = dict(keep_order=True) if keep_order else {}
    edited, fresh = new_mesh(contexts[single], 256, CONFIGS[cfg], **kw), new_mesh(contexts[single], 300, CONFIGS[cfg], **kw)
    edited.resize(300)
    for name, a, b in zip(("cov_bound", "block_box", "position"), planes(edited, 300), planes(fresh, 300)):
        assert a == b, name
    # ... and it takes splats behind its old capacity
    extra = scene_data(290, CONFIGS[cfg]["deg"], 77, CONFIGS[cfg]["u8"])
    for m in (edited, fresh):
        m.build(*[a if a.size else None for a in extra])
    same_as_fresh(edited, fresh, 300)
    edited.dispose()
    fresh.dispose()


def test_later_operations_behave_as_on_the_fresh_mesh(ctx):
    cfg = CONFIGS["sh2_fp16"]
    edited, fresh, runs = resize_case(ctx, (300, 257, 443), (1000, 1400), cfg)
    # an upload behind the old end is a fresh run
    extra = scene_data(333, 2, 77)
    for m in (edited, fresh):
        m.build(*extra, start=1000)
    same_as_fresh(edited, fresh, 1400)
    # ... which can go again on its own, and so can a run that was there before the resize
    for m in (edited, fresh):
        m.remove([(1000, 333)])
    same_as_fresh(edited, fresh, 1400)
    for m in (edited, fresh):
        m.remove([(300, 257)])
    same_as_fresh(edited, fresh, 1400)
    # the runs that are left fold into one
    for m in (edited, fresh):
        m.reorder(0, 743)
    same_as_fresh(edited, fresh, 1400)
    # and the memory of what went away is given back
    edited.resize(743)
    small = new_mesh(ctx, 743, cfg)
    upload_runs(small, [runs[0], runs[2]])
    small.reorder(0, 743)
    same_as_fresh(edited, small, 743)
    for m in (edited, fresh, small):
        m.dispose()


def test_a_dynamic_mesh_keeps_its_scene_indexes_and_takes_new_ones(ctx):
    cfg, sizes = CONFIGS["sh0_fp32"], (300, 257, 443)
    runs = [scene_data(n, 0, 60 + k) for k, n in enumerate(sizes)]
    t = [np.eye(4), np.eye(4), np.eye(4)]
    t[0][:3, 3], t[1][:3, 3], t[2][:3, 3] = (0.2, 0.0, 0.0), (0.0, 0.4, 0.0), (-0.3, 0.1, 0.2)
    t = [m.T.reshape(16) for m in t]                       # column-major
    edited, fresh = new_mesh(ctx, 557, cfg, dynamic_mode=True), new_mesh(ctx, 1100, cfg, dynamic_mode=True)
    upload_runs(edited, runs[:2], scene_of=[0, 1])
    edited.set_scenes(transforms=t[:2])
    edited.render()
    edited.resize(1100)
    upload_runs(fresh, runs[:2], scene_of=[0, 1])
    fresh.set_scenes(transforms=t[:2])
    same_as_fresh(edited, fresh, 1100)                     # (the scene parameters stayed)
    for m in (edited, fresh):
        m.build(*[a if a.size else None for a in runs[2]], start=557, scene_indexes=np.full(443, 2, np.uint32))
        m.set_scenes(transforms=t)
    same_as_fresh(edited, fresh, 1100)
    assert np.array_equal(edited._scene_of, fresh._scene_of)
    moved = new_mesh(ctx, 1100, cfg, dynamic_mode=True)    # (the indexes matter: with scene 0's for the last run the frame differs)
    upload_runs(moved, runs, scene_of=[0, 1, 0])
    moved.set_scenes(transforms=t)
    order = np.arange(1000, dtype=np.uint32)
    assert frames(moved, order)[0] != frames(fresh, order)[0]
    for m in (edited, fresh, moved):
        m.dispose()


def test_destination_draw_mode_and_deep_switch_survive(ctx):
    cfg = CONFIGS["sh0_fp32"]
    runs = runs_of((300, 257, 443), cfg)
    back = np.random.default_rng(8).integers(0, 256, size=(64, 64, 4), dtype=np.uint8)
    edited, fresh, plain = new_mesh(ctx, 1000, cfg), new_mesh(ctx, 3000, cfg), new_mesh(ctx, 3000, cfg)
    order = np.random.default_rng(4).permutation(1000).astype(np.uint32)
    for m in (edited, fresh, plain):
        upload_runs(m, runs)
        m.update_render_indexes(order, 1000)
    for m in (edited, fresh):
        m.set_destination(rgba=back)
        m.set_draw_mode(rop8=True)
        m.set_deep_pass(False)
    edited.render()
    edited.resize(3000)
    a, b, c = edited.render()[0], fresh.render()[0], plain.render()[0]
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert edited.deep_pass_info()["bins"].size == 0
    for m in (edited, fresh):
        m.set_destination()
    same_as_fresh(edited, fresh, 3000)
    for m in (edited, fresh, plain):
        m.dispose()


def test_the_same_capacity_forgets_nothing(ctx):
    cfg = CONFIGS["sh0_fp32"]
    mesh = new_mesh(ctx, 1100, cfg)
    upload_runs(mesh, runs_of((300, 257, 443), cfg))
    order = np.random.default_rng(3).permutation(1000).astype(np.uint32)
    mesh.update_render_indexes(order, 1000)
    frame = mesh.render()[0]
    ids, depth = mesh.surface(0, 0, 64, 64)
    mesh.resize(1100)
    again = mesh.surface(0, 0, 64, 64)                     # (still answers for the last draw)
    assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == depth.tobytes()
    assert mesh.render()[0].tobytes() == frame.tobytes() and mesh.max_splat_count == 1100
    mesh.resize(1200)
    with pytest.raises(GsError, match="no draw yet"):      # another capacity: the last draw is gone
        mesh.surface(0, 0, 64, 64)
    mesh.dispose()


def test_refusals_change_nothing(ctx):
    cfg = CONFIGS["sh0_fp32"]
    mesh = new_mesh(ctx, 1100, cfg)
    upload_runs(mesh, runs_of((300, 257, 443), cfg))
    order = np.random.default_rng(3).permutation(1000).astype(np.uint32)
    before = (planes(mesh, 1100), frames(mesh, order))
    for capacity, why in [(0, "max_splat_count == 0"), ((1 << 28) + 1, "2\\^28"), (999, "uploaded count 1000"), (1, "uploaded count 1000")]:
        with pytest.raises(GsError, match=why) as e:
            mesh.resize(capacity)
        assert e.value.status == L.GS_ERR_INVALID
        assert mesh.splat_count == 1000 and mesh.max_splat_count == 1100
        ids = mesh.surface(0, 0, 64, 64)[0]                # (the last draw is still there)
        assert ids.shape == (64, 64)
        assert (planes(mesh, 1100), frames(mesh, order)) == before, capacity
    with pytest.raises(GsError, match="max_splat_count"):  # the capacity still bounds an upload
        mesh.build(*[a if a.size else None for a in scene_data(101, 0, 9)], start=1000)
    mesh.dispose()


def test_the_tail_behind_the_uploaded_splats_is_a_fresh_meshs(ctx):
    """selector 12 reads up to the uploaded count: an upload at the far end of the new capacity raises it over the positions the
    resize wrote and nobody uploaded - the identity permutation, zero planes - and they are read directly"""
    cfg = CONFIGS["sh2_fp16"]
    edited, fresh, _ = resize_case(ctx, (300, 257, 443), (1000, 1400), cfg)
    far = scene_data(100, 2, 91)
    for m in (edited, fresh):
        m.build(*far, start=1300)
    pos = np.empty(1400, np.uint32)
    L.check(edited.lib.gs_mesh_debug_read(edited.handle, 12, pos.ctypes.data, 1400))
    assert np.array_equal(pos[1000:1300], np.arange(1000, 1300, dtype=np.uint32))
    bound = np.empty(1400, np.float32)
    L.check(edited.lib.gs_mesh_debug_read(edited.handle, 10, bound.ctypes.data, 1400))
    assert not bound[1000:1300].any() and bound[:1000].any()
    for name, a, b in zip(("cov_bound", "block_box", "position"), planes(edited, 1400), planes(fresh, 1400)):
        assert a == b, name
    order = np.random.default_rng(5).permutation(1400).astype(np.uint32)       # (names the never-uploaded splats too)
    for name, a, b in zip(("fp32", "rop8", "rop8_full", "surface_ids", "surface_depth"), frames(edited, order), frames(fresh, order)):
        assert a == b, name
    edited.dispose()
    fresh.dispose()


# (new capacity, bytes the allocations may grow by over what the process held when the call began): the capacity-sized scratch
# of 1000 splats is ~17 MB - the entry buffers - and is released first, so 150 000 splats' planes (88 bytes each, 13 MB) fit and
# the failure comes among the new scratch buffers, while 2 000 000 splats' planes (176 MB) fail among the planes themselves
OUT_OF_MEMORY = {"scratch_fails": (150_000, 0), "planes_fail": (2_000_000, 0), "planes_fail_later": (2_000_000, 64 << 20)}


@pytest.mark.parametrize("case", list(OUT_OF_MEMORY), ids=list(OUT_OF_MEMORY))
def test_out_of_memory_leaves_the_mesh_as_it_was(ctx, monkeypatch, case):
    """$GSPLAT_ALLOC_HEADROOM fails allocations beyond a budget counted from the bytes held when the call began.  The recovery
    must fit into what the mesh held before - so everything the call allocated is released before the old scratch comes back -
    and the mesh then draws the same bytes at the same capacity."""
    capacity, headroom = OUT_OF_MEMORY[case]
    cfg = CONFIGS["sh2_fp16"]
    mesh = new_mesh(ctx, 1000, cfg)
    runs = runs_of((300, 257, 443), cfg)
    upload_runs(mesh, runs)
    order = np.random.default_rng(3).permutation(1000).astype(np.uint32)
    before = (planes(mesh, 1000), frames(mesh, order))
    monkeypatch.setenv("GSPLAT_ALLOC_HEADROOM", f"{headroom}:{case}")
    with pytest.raises(GsError, match="GSPLAT_ALLOC_HEADROOM") as e:
        mesh.resize(capacity)
    assert e.value.status == L.GS_ERR_NOMEM
    assert mesh.max_splat_count == 1000 and mesh.splat_count == 1000
    with pytest.raises(GsError, match="no draw yet"):      # (the last draw is forgotten: the header says so)
        mesh.surface(0, 0, 64, 64)
    assert (planes(mesh, 1000), frames(mesh, order)) == before                     # still under the budget: nothing more is held
    with pytest.raises(GsError, match="max_splat_count"):
        mesh.build(*scene_data(10, 2, 9), start=1000)
    monkeypatch.delenv("GSPLAT_ALLOC_HEADROOM")
    mesh.resize(capacity)                                  # ... and with memory to be had, the same call goes through
    fresh = new_mesh(ctx, capacity, cfg)
    upload_runs(fresh, runs)
    same_as_fresh(mesh, fresh, capacity)
    mesh.dispose()
    fresh.dispose()


def test_under_poisoned_allocations_in_a_child_process():
    """resize up, upload, draw, a visibility-culled sort, resize down, draw - with every new allocation holding 0xFF: nothing may
    read memory the resize allocated and nobody wrote"""
    env = dict(os.environ, GSPLAT_POISON_ALLOC="0xFF")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "tools", "resize_child.py")], env=env, text=True, timeout=120)
    assert out.strip().splitlines()[-1] == "resize_child: ok"
