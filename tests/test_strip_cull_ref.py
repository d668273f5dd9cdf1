"""CPU tier of the strip / block cull checks: the host model (strip_cull_ref.py) against a per-splat loop and the raster oracle,
the bounds' claim in fp64 on the case list (strip_cull_cases.py), and proof that the cases bite."""
import numpy as np
import pytest

import oracle
import raster_cases
import strip_cull_cases as cases
import strip_cull_ref as ref
import test_raster_ref as raster_ref


# -- strip_planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip", [(0, 0), (5, 5), (13, 13), (0, 1), (6, 7), (12, 13), (0, 13), (3, 9), (11, 13)])
def test_strip_planes_equal_a_per_splat_loop(strip):
    """Random full-frame planes on a 20 x 13 tile grid: empty strips, one-row strips, the last (partial) row, the whole frame."""
    rng = np.random.default_rng(11)
    n = 3000
    vis = rng.random(n) < 0.7
    x = np.sort(rng.integers(0, 20, size=(n, 2)), axis=1)
    y = np.sort(rng.integers(0, 13, size=(n, 2)), axis=1)
    rects = np.stack([x[:, 0] | (y[:, 0] << 16), x[:, 1] | (y[:, 1] << 16)], axis=1).astype(np.uint32)
    rects[~vis] = ref.RECT_EMPTY
    recs = rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    recs[~vis] = 0
    r0, r1 = strip
    mask, got_rects, got_recs = ref.strip_planes(vis, rects, recs, r0, r1)
    for i in range(n):
        inside = bool(vis[i]) and y[i, 0] <= r1 - 1 and y[i, 1] >= r0 and r1 > r0      # (an empty strip holds no pixel row)
        assert mask[i] == inside
        if inside:
            assert got_rects[i].tolist() == [x[i, 0] | (max(y[i, 0], r0) << 16), x[i, 1] | (min(y[i, 1], r1 - 1) << 16)]
            assert np.array_equal(got_recs[i], recs[i])
        else:
            assert got_rects[i].tolist() == list(ref.RECT_EMPTY) and not got_recs[i].any()
    if r1 == r0:
        assert not mask.any()
    elif strip == (0, 13):
        assert np.array_equal(mask, vis) and np.array_equal(got_rects, rects) and np.array_equal(got_recs, recs)
    else:
        assert 0 < mask.sum() < vis.sum()


# -- vertical_extent --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", raster_cases.CASES)
def test_vertical_extent_matches_the_raster_oracle(name):
    """The restatement against oracle.project (itself pinned to the reference's shader text) on the raster cases, at the tolerance
    test_raster_ref.py states for the basis.  The fp64 evaluation - the one the bound checks below use - is held there in what
    they read: its vertical extent raw = sqrt(b1y^2 + b2y^2), hence ext_y, and the quad's diagonal.  The four basis components
    are compared in the oracle's precision as well (the same statements evaluated in fp32): where l1 - a cancels, fp32 and fp64
    disagree in the direction of a long needle, a property of the shader's arithmetic and not of the restatement, and the long
    axis of such a needle is still held by raw."""
    case = raster_cases.make_case(name)
    un = case["uniforms"]
    u = ref.uniforms(case["camera"], focal_adjustment=1.0 / un["inverse_focal_adjustment"], splat_scale=un["splat_scale"],
                     kernel2d=case["kernel2d"], max_splat_px=case["max_splat_px"], antialiased=case["antialiased"],
                     point_cloud=bool(un["point_cloud"]), dynamic=case["build"] == "dynamic2")
    view = view32 = None
    if u.dynamic:
        view = ref.scene_views(u.view_matrix, un["transforms"])[case["scene_idx"]]
        view32 = ref.scene_views(u.view_matrix, un["transforms"], np.float32)[case["scene_idx"]]
    sh = None
    if case["sh_stored"]:
        sh = case["sh_u8"].astype(np.float32) if case["sh8"] else case["sh_sampled"]
    o = oracle.project(raster_ref._oracle_camera(case), case["centers"], case["cov"], case["rgba"], sh, scene_indexes=case["scene_idx"])
    k = o["visible"] == 1
    e = ref.vertical_extent(u, case["centers"], case["cov"], view32, dtype=np.float32)
    e64 = ref.vertical_extent(u, case["centers"], case["cov"], view)
    assert k.sum() > 100 and e.ok[k].all() and e64.ok[k].all()
    atol = 1e-4 * max(un["viewport"]) / 100
    for col in ("b1x", "b1y", "b2x", "b2y"):
        np.testing.assert_allclose(getattr(e, col)[k], o[col][k], rtol=2e-4, atol=atol)
    want_raw = np.hypot(o["b1y"][k].astype(np.float64), o["b2y"][k])
    np.testing.assert_allclose(e.raw[k], want_raw, rtol=2e-4, atol=atol)
    np.testing.assert_allclose(e64.raw[k], want_raw, rtol=2e-4, atol=atol)                       # fp64: the vertical extent itself
    np.testing.assert_allclose(e64.ext_y[k], want_raw * 1.00001 + 1e-3, rtol=2e-4, atol=atol)   # and its padded value
    # |e1| = 1 keeps the quad's diagonal sqrt(h1^2 + h2^2) k independent of the direction
    diag = lambda r: np.sqrt(np.asarray(r["b1x"], dtype=np.float64) ** 2 + np.asarray(r["b1y"], dtype=np.float64) ** 2
                             + np.asarray(r["b2x"], dtype=np.float64) ** 2 + np.asarray(r["b2y"], dtype=np.float64) ** 2)
    np.testing.assert_allclose(diag(vars(e64))[k], diag(o)[k], rtol=2e-4, atol=atol)
    cy, ok = ref.window_y(u, case["centers"], view)
    assert ok[k].all()
    np.testing.assert_allclose(cy[k], o["cy"][k], rtol=0, atol=2e-3)


# -- the bounds on the case list --------------------------------------------------------------------------------------------------
_MODELS = {}


def model(name):
    """Per case, computed once: uniforms, what the full test keeps, ext_y, the covariance values read, storage blocks."""
    if name not in _MODELS:
        c = cases.make_case(name)
        u = cases.model_uniforms(c)
        centers, cov, view = cases.final_centers(c), cases.cov_read(c), cases.splat_views(c, u)
        e = ref.vertical_extent(u, centers, cov, view)
        _, ok = ref.window_y(u, centers, view)
        bound32 = ref.cov_bound(cov).astype(np.float32)
        pos = cases.morton_positions(c.centers, c.uploads)
        boxes = ref.block_boxes(centers, bound32, pos, (c.count + 255) // 256)
        _MODELS[name] = (c, u, centers, cov, view, e, ok & e.ok, bound32, boxes)
    return _MODELS[name]


def shortfall(name, weaken=None):
    """max over the kept splats of ext_y - reach (positive: the pre-test may drop a splat the exact test keeps)."""
    c, u, centers, cov, view, e, kept, bound32, _ = model(name)
    bound = ref.cov_bound(cov, weaken) if weaken == "trace_bound" else bound32
    reach = ref.splat_reach(u, centers, bound, weaken)
    assert kept.sum() > 500, "the case keeps too few splats to say anything"
    return float((e.ext_y[kept] - reach[kept]).max())


@pytest.mark.parametrize("name", cases.NAMES)
def test_reach_covers_the_vertical_extent(name):
    """(a) The bound's claim, in fp64: splat_reach >= ext_y for every splat the full test keeps."""
    assert shortfall(name) <= 0.0


@pytest.mark.parametrize("weaken", ref.WEAKENINGS)
def test_each_weakening_of_the_bound_is_caught(weaken):
    """(b) Dropping the + 0.3163, bounding the spectral radius by trace / 3, or dropping row 2 of mat3(modelView) from |T0|, |T1|
    makes (a) fail on at least two cases: the cases reach each term of the bound, and go on reaching it if one of them changes."""
    worst = {name: shortfall(name, weaken) for name in cases.NAMES}
    assert sum(w > 0.5 for w in worst.values()) >= 2, worst    # by more than the half pixel the exact rect clip forgives


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_cases_exercise_both_culls(name):
    """(c) In some cut of the frame the model's pre-test drops at least 50 splats that pass the frustum, and its block strip test
    declares at least 4 blocks dead - or none at all where the block test must stand down (orthographic, per-scene transforms)."""
    c, u, centers, cov, view, e, kept, bound32, boxes = model(name)
    _, frustum_ok = ref.window_y(u, centers, view)
    dropped = [int((frustum_ok & ~ref.pretest_keeps(u, centers, bound32, r0, r1, view=view)).sum()) for r0, r1 in cases.CUTS]
    dead = [int(ref.block_dead(u, boxes, r0, r1)[1].sum()) for r0, r1 in cases.CUTS]
    assert max(dropped) >= 50, dropped
    assert (max(dead) >= 4) if c.block_strip else (max(dead) == 0), dead
    # and the bound matters: splats kept by the exact test of a cut whose centre lies outside it
    cy, _ = ref.window_y(u, centers, view)
    outside_but_kept = max(int((kept & ((cy + e.ext_y >= 16 * r0 + 0.5) & (cy < 16 * r0 - 4) | (cy - e.ext_y <= 16 * r1 - 0.5) & (cy > 16 * r1 + 4))).sum())
                           for r0, r1 in cases.CUTS)
    assert outside_but_kept >= 50, outside_but_kept


def test_case_shapes():
    sizes = {name: cases.make_case(name).count for name in cases.NAMES}
    assert all(4000 <= s <= 20000 and s % 256 for s in sizes.values()) and sizes["needles"] % 256 == 1
    assert cases.ROWS == 13 and cases.H % 16 != 0 and len(cases.STRIPS) == 15 and set(cases.CUTS) <= set(cases.STRIPS)
