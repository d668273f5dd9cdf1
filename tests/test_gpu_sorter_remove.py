"""-m gpu: gs_sorter_remove held to its definition - afterwards every sort's list is, bit for bit, the list of a fresh sorter of
the same capacity and flags that received the surviving centres at their new positions.  Three scenes; the one that goes holds the
extreme points of the hull in the integer cases, so a key range (or 16-bit centre planes) left over from it would change the
bucket of every key and the order of the ties.  A sort runs before the removal, so that the caches, the stale-key state and the
16-bit key path are populated.  With a bound mesh: the visibility cull, a rebuilt tree's gather, the lists and the frames equal a
fresh mesh, sorter and tree, in both orders of the two remove calls and with a draw between them."""
import numpy as np
import pytest

import helpers
import oracle
from gaussiansplats3d_amd import Context, GsError, SplatMesh, SplatTree, camera, create_sort_worker, util
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
SIZES = (300, 257, 443)
GONE = (300, 257)                                          # the middle scene
CAPACITY = 1100


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def three_scenes(seed=21):
    """[(centres float32 [n, 3])] - scene 1 blown up about the common mean: every extreme point of the hull is one of its splats"""
    cs = [helpers.small_scene(n, 0, seed + k).centers for k, n in enumerate(SIZES)]
    mean = np.concatenate(cs).mean(axis=0)
    cs[1] = ((cs[1] - mean) * np.float32(4.0) + mean).astype(np.float32)
    allc = np.concatenate(cs)
    for axis in range(3):
        assert 300 <= int(allc[:, axis].argmin()) < 557 and 300 <= int(allc[:, axis].argmax()) < 557
    return cs


def transforms3():
    t = [np.eye(4, dtype=np.float32) for _ in range(3)]
    t[0][:3, 3], t[1][:3, 3], t[2][:3, 3] = (0.2, 0.0, 0.1), (0.0, 0.4, -0.3), (-0.3, 0.1, 0.5)
    return [m.T.reshape(16) for m in t]                    # column-major


def upload(worker, scenes, scene_ids, integer):
    at = 0
    for c, sid in zip(scenes, scene_ids):
        aos = util.integer_centers(c) if integer else util.float_centers(c)
        worker.post_message({"centers": aos, "sceneIndexes": np.full(len(c), sid, np.uint32),
                             "range": {"from": at, "to": at + len(c) - 1, "count": len(c)}})
        at += len(c)
    return at


def sort_list(worker, mvp, n, transforms=None, indexes=None, sort_count=None):
    msg = {"modelViewProj": mvp, "splatRenderCount": n, "splatSortCount": n if sort_count is None else sort_count, "indexesToSort": indexes}
    if transforms is not None:
        msg["transforms"] = np.concatenate(transforms)
    return worker.post_message({"sort": msg})["sortedIndexes"]


def sorter_case(ctx, integer, dynamic):
    scenes, cam = three_scenes(), camera.demo_camera("garden", 64, 64)
    mvp, t = cam.sort_mvp(), transforms3() if dynamic else None
    kw = dict(integer_based_sort=integer, dynamic_mode=dynamic)
    edited, fresh = create_sort_worker(ctx, CAPACITY, **kw), create_sort_worker(ctx, CAPACITY, **kw)
    try:
        assert upload(edited, scenes, [0, 1, 2], integer) == 1000
        before = sort_list(edited, mvp, 1000, t)           # populates the caches and, static integer, the 16-bit key path
        range_before = edited.debug_read(4, 8)
        edited.post_message({"remove": {"ranges": [GONE], "sceneRemap": [0, 0, 1] if dynamic else None}})
        assert edited.uploaded_splat_count == 743
        with pytest.raises(GsError, match="no sort has run"):                      # the result of the old numbering is gone
            edited.debug_read(2, 10)
        kept = [scenes[0], scenes[2]]
        assert upload(fresh, kept, [0, 1], integer) == 743
        t2 = [t[0], t[2]] if dynamic else None
        got, want = sort_list(edited, mvp, 743, t2), sort_list(fresh, mvp, 743, t2)
        assert got.tobytes() == want.tobytes()
        assert sorted(got.tolist()) == list(range(743)) and before.size == 1000
        if integer and not dynamic:
            ci = util.integer_centers(np.concatenate(kept))
            assert np.array_equal(got, oracle.sort_indexes(np.arange(743, dtype=np.uint32), ci, mvp))
            # the front end saw the survivors' key range - not the one the removed hull gave - and took the same path
            a, b = edited.debug_read(4, 8), fresh.debug_read(4, 8)
            assert a[0] == b[0] == 1 and (a[2], a[3], a[6], a[7]) == (b[2], b[3], b[6], b[7]), (a, b)
            assert (range_before[2], range_before[3]) != (a[2], a[3]) and range_before[3] - range_before[2] > a[3] - a[2]
        # partial sorts through a host index list
        idx = np.random.default_rng(2).permutation(743)[:600].astype(np.uint32)
        for sort_count in (600, 250):
            got = sort_list(edited, mvp, 600, t2, indexes=idx, sort_count=sort_count)
            want = sort_list(fresh, mvp, 600, t2, indexes=idx, sort_count=sort_count)
            assert got.tobytes() == want.tobytes(), sort_count
        # a second removal, in front, and an upload behind: still a fresh sorter's lists
        edited.remove([(0, 300)], scene_remap=[0, 0] if dynamic else None)
        at = 443
        for w, first in ((edited, 443), (fresh, None)):
            if first is None:
                w.terminate()
                w = fresh = create_sort_worker(ctx, CAPACITY, **kw)
                upload(w, [scenes[2]], [0], integer)
            aos = util.integer_centers(scenes[0]) if integer else util.float_centers(scenes[0])
            w.post_message({"centers": aos, "sceneIndexes": np.full(300, 1, np.uint32), "range": {"from": at, "to": at + 299, "count": 300}})
        t3 = [t[2], t[0]] if dynamic else None
        assert sort_list(edited, mvp, 743, t3).tobytes() == sort_list(fresh, mvp, 743, t3).tobytes()
    finally:
        edited.terminate()
        fresh.terminate()


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "float"])
def test_lists_after_a_removal_are_a_fresh_sorters(ctx, integer, dynamic):
    sorter_case(ctx, integer, dynamic)


def test_refusals_change_nothing(ctx):
    scenes, cam = three_scenes(), camera.demo_camera("garden", 64, 64)
    w = create_sort_worker(ctx, CAPACITY)
    upload(w, scenes, [0, 0, 0], True)
    before = sort_list(w, cam.sort_mvp(), 1000)
    for ranges, remap, why in [([(557, 443), (0, 300)], None, "ascending"), ([(5, 0)], None, "empty"), ([(557, 544)], None, "max_splat_count"),
                               ([(k, 1) for k in range(33)], None, "GS_MAX_SCENES"), ([(0, 3)], [40], "scene_remap")]:
        with pytest.raises(GsError, match=why) as e:
            w.remove(ranges, scene_remap=remap)
        assert e.value.status == L.GS_ERR_INVALID and w.uploaded_splat_count == 1000
        assert w.debug_read(2, 1000).tobytes() == before.tobytes()                 # the resident result is still there
    w.remove([])
    w.remove([(1000, 100)])                                # behind the uploaded centres: nothing to remove
    assert w.debug_read(2, 1000).tobytes() == before.tobytes()
    w.remove([(10, 5), (700, 100)])                        # a sorter has no runs: any range
    assert w.uploaded_splat_count == 895
    fresh = create_sort_worker(ctx, CAPACITY)
    allc = np.concatenate(scenes)
    upload(fresh, [allc[np.r_[0:10, 15:700, 800:1000]]], [0], True)
    assert sort_list(w, cam.sort_mvp(), 895).tobytes() == sort_list(fresh, cam.sort_mvp(), 895).tobytes()
    w.terminate()
    fresh.terminate()


class Trio:
    """a mesh, a sorter bound to it and a tree over the same splats"""

    def __init__(self, ctx, scenes, cam, seeds):
        self.cam, self.mvp = cam, cam.sort_mvp()
        self.mesh = SplatMesh(ctx, CAPACITY, 0)
        self.worker = create_sort_worker(ctx, CAPACITY)
        self.tree = None
        at = 0
        for k, c in enumerate(scenes):
            s = helpers.small_scene(len(c), 0, seeds[k])   # (covariances and colours; the centres are the scene's)
            self.mesh.build(c, s.cov, s.rgba, None, start=at)
            at += len(c)
        upload(self.worker, scenes, [0] * len(scenes), True)
        self.mesh.set_camera(cam)
        self.mesh.use_sorter_result(self.worker, at)       # binds
        self.n = at

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

    def close(self):
        for o in (self.tree, self.worker, self.mesh):
            if o is not None:
                (o.terminate if o is self.worker else o.dispose)()


@pytest.mark.parametrize("mesh_first", [True, False], ids=["mesh_first", "sorter_first"])
def test_a_bound_mesh_sorter_and_tree(ctx, mesh_first):
    scenes, cam = three_scenes(), camera.demo_camera("garden", 64, 64)
    kept = [scenes[0], scenes[2]]
    edited, fresh = Trio(ctx, scenes, cam, (21, 22, 23)), Trio(ctx, kept, cam, (21, 23))
    try:
        edited.plant(ctx, np.concatenate(scenes))
        edited.culled_frame()                              # resident result, derived mask, position map: all of the old numbering
        edited.gathered_frame()                            # ... and the per-tree caches
        edited.tree.gather_scene_nodes_for_sort(cam, sort_worker=edited.worker, to_host=False)   # a gathered list is pending
        calls = [lambda: edited.mesh.remove([GONE]), lambda: edited.worker.remove([GONE])]
        calls[0 if mesh_first else 1]()
        # between the two calls: the sorter's result is gone, and a draw from a host list is safe - even one that still names
        # splats at or beyond the mesh's count
        with pytest.raises(GsError, match="no device-resident result"):
            edited.mesh.render()
        with pytest.raises(GsError, match="no gs_tree_gather has filled"):
            edited.worker.sort_gathered(edited.mvp)
        n_mesh = 743 if mesh_first else 1000
        edited.mesh.update_render_indexes(np.arange(1000, dtype=np.uint32)[::-1].copy(), n_mesh)
        between = edited.mesh.render()[0]
        assert between.any()
        if not mesh_first:                                 # the sorter already sorts the 743 it has, the mesh still draws them
            edited.worker.sort_on_device(edited.mvp, 743)
            edited.mesh.use_sorter_result(edited.worker, 743)
            edited.mesh.render()
        calls[1 if mesh_first else 0]()
        edited.n = 743
        edited.mesh.use_sorter_result(edited.worker, 743)
        for trio in (edited, fresh):
            trio.plant(ctx, np.concatenate(kept))
        a, b = edited.culled_frame(), fresh.culled_frame()
        assert a[0].tobytes() == b[0].tobytes() and 0 < a[0].size <= 743
        assert a[1].tobytes() == b[1].tobytes() and a[1].any()
        a, b = edited.gathered_frame(), fresh.gathered_frame()
        for name, x, y in zip(("gathered", "sorted", "frame"), a, b):
            assert x.tobytes() == y.tobytes(), name
        a, b = edited.culled_frame(), fresh.culled_frame()                         # and once more, the caches now warm
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        edited.close()
        fresh.close()
