"""-m gpu: device memory the library reads before it writes it.  Fresh allocations usually come back zeroed, so every other test
sees zeros where the code has no right to expect them.  With $GSPLAT_POISON_ALLOC=<byte> every new allocation (DevBuf::alloc)
holds that byte instead; here fresh objects are made under it and held to the same answers as without it.

First the by-original-index visibility mask: a full-frame (lazy) projection left its fresh buffer to the sorter, which writes only
the words of the positions it sorts and then declared the whole mask clean - a later strip projection after more splats were
uploaded OR'ed its survivors into garbage, and the visibility-culled sort kept splats the vertex stage had rejected.
Then a sweep of existing oracle comparisons (their own functions, helpers and goldens) under two poison bytes."""
import numpy as np
import pytest

import helpers
import oracle
import test_gpu_deep
import test_gpu_distances
import test_gpu_frustum_cull
import test_gpu_render
import test_gpu_rop8_mode
import test_gpu_sort
import test_gpu_vis_cull
import test_tree
import kat_cases
from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, util

pytestmark = pytest.mark.gpu


def _poisoned_context(monkeypatch, byte):
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", hex(byte))     # (read at every allocation: stays set for the whole test)
    return Context(0)


@pytest.fixture(params=[0xFF, 0x5A], ids=["ff", "5a"])
def pctx(request, monkeypatch):
    c = _poisoned_context(monkeypatch, request.param)
    yield c
    c.close()


def test_strip_after_a_lazy_sort_and_an_upload_keeps_only_the_strip_survivors(monkeypatch):
    ctx = _poisoned_context(monkeypatch, 0xFF)
    n = 40000
    scene = helpers.small_scene(2 * n, 1, seed=61)
    cam = camera.demo_camera("garden", 640, 360)
    mvp = cam.sort_mvp()
    ci = util.integer_centers(scene.centers)
    worker = create_sort_worker(ctx, 2 * n)
    worker.post_message({"centers": ci[:n], "range": {"from": 0, "to": n - 1, "count": n}})
    mesh = SplatMesh(ctx, 2 * n, 1)
    mesh.build(scene.centers[:n], scene.cov[:n], scene.rgba[:n], scene.sh[:n])
    mesh.set_camera(cam)
    worker.sort_on_device(mvp, n)
    mesh.use_sorter_result(worker, n)                    # binds the sorter to the mesh
    worker.sort_on_device(mvp, n)
    mesh.render()
    _, _, vis = mesh.debug_records()
    assert 1000 < vis.sum() < n

    def culled(count, strip=None):
        mesh.project(strip)
        reply = worker.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": count, "splatSortCount": count}})
        mesh.render(tile_rows=strip)
        return reply["sortedIndexes"].copy(), int(reply["stats"].result_count)

    worker.set_visibility_cull(True)
    order = oracle.sort_indexes(np.arange(n, dtype=np.uint32), ci[:n], mvp)
    got, kept = culled(n)                                # full frame: the sorter derives the mask (lazy)
    np.testing.assert_array_equal(got, order[vis[order]])
    assert kept == int(vis.sum())

    # the rest of the splats arrive; a plain draw, then a strip (a strip's projection sets the mask bits itself)
    mesh.build(scene.centers[n:], scene.cov[n:], scene.rgba[n:], scene.sh[n:], start=n)
    worker.post_message({"centers": ci[n:], "range": {"from": n, "to": 2 * n - 1, "count": n}})
    worker.set_visibility_cull(False)
    worker.sort_on_device(mvp, 2 * n)
    mesh.use_sorter_result(worker, 2 * n)
    mesh.render()
    worker.set_visibility_cull(True)
    rows = (cam.height + 15) // 16
    strip = (rows // 3, 2 * rows // 3)
    got, kept = culled(2 * n, strip)
    _, _, vis_strip = mesh.debug_records()               # the strip's vertex-stage survivors
    assert 100 < vis_strip.sum() < 2 * n
    order2 = oracle.sort_indexes(np.arange(2 * n, dtype=np.uint32), ci, mvp)
    expect = order2[vis_strip[order2]]
    extra = np.setdiff1d(got, expect)
    assert extra.size == 0, f"{extra.size} splats the vertex stage rejected were kept (first: {extra[:8]})"
    np.testing.assert_array_equal(got, expect)
    assert kept == int(vis_strip.sum())
    worker.terminate()
    mesh.dispose()
    ctx.close()


# ------------------------------------------------------------------------------ the sweep: existing comparisons, fresh poisoned objects
SORT_KATS = ["two", "range_plus_1", "permuted_partial", "p20", "float_dynamic", "pre_float"]


@pytest.mark.parametrize("name", SORT_KATS)
def test_sort_kats(pctx, name):
    case = next(c for c in kat_cases.CASES if c["name"] == name)
    test_gpu_sort.test_reference_goldens_bit_exact(pctx, case)


@pytest.mark.parametrize("sh_degree,cov_half,w,h", [(2, False, 256, 144), (2, True, 320, 200)])
def test_framebuffer(pctx, sh_degree, cov_half, w, h):
    test_gpu_render.test_framebuffer_matches_oracle(pctx, sh_degree, cov_half, w, h)


def test_strips_tile_the_frame(pctx):
    test_gpu_render.test_tile_row_strips_tile_the_full_frame(pctx)


def test_deep_pass_on_and_off(pctx):
    test_gpu_deep.test_deep_pass_and_per_bin_kernel_produce_the_same_bits(pctx)


def test_rop8_window(pctx):
    test_gpu_rop8_mode.test_rop8_draw_matches_the_rop_emulating_oracle_on_every_pixel(pctx, 2, False, 320, 200, 20000, False)


def test_frustum_culled_sort(pctx):
    test_gpu_frustum_cull.test_culled_sort_is_the_reference_sort_with_dropped_splats_removed(pctx, "garden", True, 16, 50000)


def test_visibility_culled_sort(pctx):
    test_gpu_vis_cull.test_visibility_culled_sort_is_the_reference_list_restricted_to_what_the_frame_draws(pctx)


def test_visibility_culled_sort_with_a_derived_mask(pctx):
    test_gpu_vis_cull.test_full_frame_projection_leaves_the_original_order_mask_to_the_sorter(pctx)


def test_tree_gather(pctx):
    name, k = test_tree._gather_cases()[0]
    test_tree.test_device_gather_matches_the_reference_gather(pctx, name, k)


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
def test_distances(pctx, keep_order):
    test_gpu_distances.test_distances_bit_exact(pctx, 100_003, keep_order)
