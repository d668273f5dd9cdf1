"""-m gpu: gs_sorter_resize held to its definition - after the resize and the upload of a further scene every sort is, bit for
bit, the sort of a fresh sorter of the new capacity and the same flags that received the same centres by the same uploads.  Two
scenes are resident and sorted once (caches, stale-key state, the 16-bit key path and the 16-bit centre planes are populated);
the third arrives after the resize.  The hull of all centres belongs to a resident scene in one case and to the added one in the
other: the extreme set is kept over the resize and extended by the upload, never rebuilt from rows read back.  With a bound mesh:
the visibility cull, a new tree's gather and the device distance pass equal a fresh mesh, sorter and tree, in both orders of the
two resize calls."""
import numpy as np
import pytest

import helpers
import oracle
from gaussiansplats3d_amd import Context, GsError, SplatMesh, SplatTree, camera, create_sort_worker, util
from gaussiansplats3d_amd import _lib as L
from test_gpu_sorter_remove import sort_list, transforms3, upload

pytestmark = pytest.mark.gpu
SIZES = (300, 257, 443)
PAIRS = {"1000_1001": (1000, 1001), "1000_4097": (1000, 4097), "1400_1000": (1400, 1000)}
KINDS = {"integer_static": (True, False), "integer_dynamic": (True, True), "float_static": (False, False), "float_dynamic": (False, True)}
# gs_sorter_debug_read selector 4, all eight words.  Word 5, pass 0's slot of group rows, alternates with every known-range sort
# the sorter has run: the fresh sorter runs the sort the edited one ran before its resize, so the two have the same history
FRONT_WORDS = list(range(8))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def three_scenes(hull, seed=21):
    """[(centres float32 [n, 3])] - scene `hull` blown up about the common mean: every extreme point of the hull is one of its splats"""
    cs = [helpers.small_scene(n, 0, seed + k).centers for k, n in enumerate(SIZES)]
    mean = np.concatenate(cs).mean(axis=0)
    cs[hull] = ((cs[hull] - mean) * np.float32(4.0) + mean).astype(np.float32)
    allc, lo = np.concatenate(cs), int(np.cumsum((0,) + SIZES)[hull])
    for axis in range(3):
        assert lo <= int(allc[:, axis].argmin()) < lo + SIZES[hull] and lo <= int(allc[:, axis].argmax()) < lo + SIZES[hull]
    return cs


def add_scene(worker, centres, at, scene, integer):
    aos = util.integer_centers(centres) if integer else util.float_centers(centres)
    n = len(centres)
    worker.post_message({"centers": aos, "sceneIndexes": np.full(n, scene, np.uint32), "range": {"from": at, "to": at + n - 1, "count": n}})


def sort_everything(worker, mvp, t, integer):
    """every kind of sort, each with its list, statistics and debug planes: [(name, bytes ...)]"""
    out = []
    rng = np.random.default_rng(2)
    idx = rng.permutation(1000)[:600].astype(np.uint32)
    pre = (rng.integers(-50000, 50000, 1000).astype(np.int32) if integer else rng.normal(size=1000).astype(np.float32))
    calls = [("identity", dict(n=1000)), ("host_list", dict(n=600, indexes=idx)), ("partial", dict(n=600, indexes=idx, sort_count=250)),
             ("precomputed", dict(n=1000, pre=pre))]
    for name, c in calls:
        msg = {"modelViewProj": mvp, "splatRenderCount": c["n"], "splatSortCount": c.get("sort_count", c["n"]), "indexesToSort": c.get("indexes")}
        if t is not None:
            msg["transforms"] = np.concatenate(t)
        if "pre" in c:
            msg.update(usePrecomputedDistances=True, precomputedDistances=c["pre"])
        reply = worker.post_message({"sort": msg})
        s = reply["stats"]
        stats = (s.key_min, s.key_max, s.clamped, s.passes, s.result_count)
        planes = [worker.debug_read(what, c["n"]).tobytes() for what in (0, 1, 2)] + [worker.debug_read(4, 8)[FRONT_WORDS].tobytes()]
        out.append((name, reply["sortedIndexes"].tobytes(), stats, planes))
    return out


@pytest.mark.parametrize("hull", [0, 2], ids=["hull_resident", "hull_added"])
@pytest.mark.parametrize("pair", list(PAIRS), ids=list(PAIRS))
@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
def test_sorts_after_a_resize_are_a_fresh_sorters(ctx, kind, pair, hull):
    integer, dynamic = KINDS[kind]
    old, new = PAIRS[pair]
    scenes, cam = three_scenes(hull), camera.demo_camera("garden", 64, 64)
    mvp, t = cam.sort_mvp(), transforms3() if dynamic else None
    kw = dict(integer_based_sort=integer, dynamic_mode=dynamic)
    edited, fresh = create_sort_worker(ctx, old, **kw), create_sort_worker(ctx, new, **kw)
    try:
        assert upload(edited, scenes[:2], [0, 1], integer) == 557
        before = sort_list(edited, mvp, 557, t)            # populates the caches and, static integer, the 16-bit paths
        edited.post_message({"resize": {"maxSplatCount": new}})
        assert edited.max_splat_count == new and edited.uploaded_splat_count == 557
        with pytest.raises(GsError, match="no sort has run"):                      # the result went with its buffer
            edited.debug_read(2, 10)
        upload(fresh, scenes[:2], [0, 1], integer)
        assert sort_list(fresh, mvp, 557, t).tobytes() == before.tobytes()         # (the same history of sorts: FRONT_WORDS)
        # the two scenes that were resident, before anything is uploaded again
        assert sort_list(edited, mvp, 557, t).tobytes() == sort_list(fresh, mvp, 557, t).tobytes() == before.tobytes()
        if integer and not dynamic:
            assert np.array_equal(edited.debug_read(4, 8)[FRONT_WORDS], fresh.debug_read(4, 8)[FRONT_WORDS])
        for w in (edited, fresh):
            add_scene(w, scenes[2], 557, 2, integer)
        got, want = sort_everything(edited, mvp, t, integer), sort_everything(fresh, mvp, t, integer)
        for (name, la, sa, pa), (_, lb, sb, pb) in zip(got, want):
            assert la == lb, name
            assert sa == sb, (name, sa, sb)
            for what, a, b in zip((0, 1, 2, 4), pa, pb):
                assert a == b, (name, what)
        if integer and not dynamic:
            ci = util.integer_centers(np.concatenate(scenes))
            assert got[0][1] == oracle.sort_indexes(np.arange(1000, dtype=np.uint32), ci, mvp).tobytes()
            assert np.frombuffer(got[0][3][3], np.int32)[0] == 1                   # the identity sort knew its key range
    finally:
        edited.terminate()
        fresh.terminate()


def test_refusals_change_nothing(ctx):
    scenes, cam = three_scenes(0), camera.demo_camera("garden", 64, 64)
    w = create_sort_worker(ctx, 1100)
    upload(w, scenes, [0, 0, 0], True)
    before = sort_list(w, cam.sort_mvp(), 1000)
    for capacity, why in [(0, "max_splat_count == 0"), (999, "uploaded splat count 1000"), (1, "uploaded splat count 1000")]:
        with pytest.raises(GsError, match=why) as e:
            w.resize(capacity)
        assert e.value.status == L.GS_ERR_INVALID and w.max_splat_count == 1100 and w.uploaded_splat_count == 1000
        assert w.debug_read(2, 1000).tobytes() == before.tobytes()                 # the resident result is still there
    w.resize(1100)                                         # the capacity it has: nothing happens
    assert w.debug_read(2, 1000).tobytes() == before.tobytes()
    with pytest.raises(GsError, match="max_splat_count"):  # the capacity still bounds an upload
        add_scene(w, scenes[0][:101], 1000, 0, True)
    w.resize(1000)
    with pytest.raises(GsError, match="no sort has run"):
        w.debug_read(2, 10)
    assert sort_list(w, cam.sort_mvp(), 1000).tobytes() == before.tobytes()
    w.terminate()


def test_out_of_memory_leaves_the_sorter_as_it_was(ctx, monkeypatch):
    """$GSPLAT_ALLOC_HEADROOM=0: nothing may be held beyond what was held when the call began, so the new planes fail - and the
    recovery, which releases them before it allocates the old scratch again, fits; the sorter sorts as before at its capacity"""
    scenes, cam = three_scenes(0), camera.demo_camera("garden", 64, 64)
    w = create_sort_worker(ctx, 1100)
    upload(w, scenes, [0, 0, 0], True)
    before = sort_list(w, cam.sort_mvp(), 1000)
    front = w.debug_read(4, 8)
    monkeypatch.setenv("GSPLAT_ALLOC_HEADROOM", "0:sorter")
    with pytest.raises(GsError, match="GSPLAT_ALLOC_HEADROOM") as e:
        w.resize(1_000_000)
    assert e.value.status == L.GS_ERR_NOMEM and w.max_splat_count == 1100 and w.uploaded_splat_count == 1000
    with pytest.raises(GsError, match="no sort has run"):
        w.debug_read(2, 10)
    assert sort_list(w, cam.sort_mvp(), 1000).tobytes() == before.tobytes()
    monkeypatch.delenv("GSPLAT_ALLOC_HEADROOM")
    assert sort_list(w, cam.sort_mvp(), 1000).tobytes() == before.tobytes()
    after = w.debug_read(4, 8)
    assert (after[0], after[1], after[2], after[3], after[4]) == (front[0], front[1], front[2], front[3], front[4])
    with pytest.raises(GsError, match="max_splat_count"):
        add_scene(w, scenes[0][:101], 1000, 0, True)
    w.resize(1_000_000)
    assert sort_list(w, cam.sort_mvp(), 1000).tobytes() == before.tobytes() and w.max_splat_count == 1_000_000
    w.terminate()


class Trio:
    """a mesh, a sorter bound to it and a tree over the same splats"""

    def __init__(self, ctx, capacity, scenes, cam, seeds):
        self.cam, self.mvp = cam, cam.sort_mvp()
        self.mesh = SplatMesh(ctx, capacity, 0)
        self.worker = create_sort_worker(ctx, capacity)
        self.tree = None
        self.n = 0
        self.mesh.set_camera(cam)
        for c, seed in zip(scenes, seeds):
            self.add(c, seed)

    def add(self, c, seed):
        s = helpers.small_scene(len(c), 0, seed)           # (covariances and colours; the centres are the scene's)
        self.mesh.build(c, s.cov, s.rgba, None, start=self.n)
        add_scene(self.worker, c, self.n, 0, True)
        self.n += len(c)
        self.mesh.use_sorter_result(self.worker, self.n)   # binds

    def plant(self, ctx, centres):
        if self.tree is not None:
            self.tree.dispose()
        self.tree = SplatTree(ctx, max_depth=4, max_centers_per_node=64).process_splat_mesh(centres)

    def culled_frame(self):
        """project, a visibility-culled sort whose list also comes to the host, the draw from the resident result"""
        self.worker.set_visibility_cull(True)
        self.mesh.project()
        kept = sort_list(self.worker, self.mvp, self.n)
        self.mesh.use_sorter_result(self.worker, self.n)
        frame = self.mesh.render()[0]
        self.worker.set_visibility_cull(False)
        return kept, frame

    def gathered_frame(self):
        g = self.tree.gather_scene_nodes_for_sort(self.cam, sort_worker=self.worker)
        reply = self.worker.sort_gathered(self.mvp)
        self.mesh.use_sorter_result(self.worker, g["splatRenderCount"])
        return g["indexesToSort"], reply["sortedIndexes"], self.mesh.render()[0]

    def distance_frame(self):
        """gs_mesh_compute_distances with the sorter as its destination, sorted from the device"""
        self.mesh.compute_distances_on_gpu(self.mvp, sort_worker=self.worker)
        reply = self.worker.post_message({"sort": {"modelViewProj": self.mvp, "splatRenderCount": self.n, "splatSortCount": self.n,
                                                   "usePrecomputedDistances": True, "precomputedOnDevice": True}})
        self.mesh.use_sorter_result(self.worker, self.n)
        return reply["sortedIndexes"], self.mesh.render()[0]

    def close(self):
        for o in (self.tree, self.worker, self.mesh):
            if o is not None:
                (o.terminate if o is self.worker else o.dispose)()


@pytest.mark.parametrize("mesh_first", [True, False], ids=["mesh_first", "sorter_first"])
def test_a_bound_mesh_sorter_and_tree(ctx, mesh_first):
    scenes, cam = three_scenes(2), camera.demo_camera("garden", 64, 64)
    edited, fresh = Trio(ctx, 557, scenes[:2], cam, (21, 22)), Trio(ctx, 1000, scenes, cam, (21, 22, 23))
    try:
        edited.plant(ctx, np.concatenate(scenes[:2]))
        edited.culled_frame()                              # resident result, derived mask, position map
        edited.gathered_frame()                            # ... and the per-tree caches
        edited.tree.gather_scene_nodes_for_sort(cam, sort_worker=edited.worker, to_host=False)   # a gathered list is pending
        calls = [lambda: edited.mesh.resize(1000), lambda: edited.worker.resize(1000)]
        calls[0 if mesh_first else 1]()
        # between the two calls: the sorter's result is gone, and a draw from a host list is safe
        with pytest.raises(GsError, match="no device-resident result"):
            edited.mesh.render()
        edited.mesh.update_render_indexes(np.arange(557, dtype=np.uint32)[::-1].copy(), 557)
        assert edited.mesh.render()[0].any()
        calls[1 if mesh_first else 0]()
        with pytest.raises(GsError, match="no gs_tree_gather has filled"):
            edited.worker.sort_gathered(edited.mvp)
        edited.add(scenes[2], 23)
        for trio in (edited, fresh):
            trio.plant(ctx, np.concatenate(scenes))
        a, b = edited.culled_frame(), fresh.culled_frame()
        assert a[0].tobytes() == b[0].tobytes() and 0 < a[0].size <= 1000
        assert a[1].tobytes() == b[1].tobytes() and a[1].any()
        for step in ("gathered_frame", "distance_frame", "culled_frame"):          # (the cull once more, the caches now warm)
            a, b = getattr(edited, step)(), getattr(fresh, step)()
            for k, (x, y) in enumerate(zip(a, b)):
                assert x.tobytes() == y.tobytes(), (step, k)
    finally:
        edited.close()
        fresh.close()
