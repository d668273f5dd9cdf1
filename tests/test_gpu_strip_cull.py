"""-m gpu: the strip and block culls of the vertex stage (csrc/project.hip: k_block_test / block_misses_strip, the per-splat strip
pre-test; csrc/mesh.hip: cov_spectral_bound, k_block_boxes) held to the full frame splat by splat.

A strip's mask, rects and records are a numpy function of the full frame's (strip_cull_ref.strip_planes): every comparison is
np.array_equal.  A splat that a too-tight bound drops reaches the strip with the faint tail of its footprint only, so the pixel
comparisons of the other tests would not see it; its bit in the mask is plain.  The cases (strip_cull_cases.py) are the geometries
where the bounds are tight; each is drawn under the four block-test switches and cut into every single tile row and five coarser
strips.  The upload-time planes behind the culls are read back and checked against fp64 numpy."""
import os
import subprocess
import sys

import numpy as np
import pytest

import strip_cull_cases as cases
import strip_cull_ref as ref
from gaussiansplats3d_amd import Context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def case_of(name):
    if name not in _CASES:
        _CASES[name] = cases.make_case(name)
    return _CASES[name]


_FULL = {}


def full_frame_without_block_cull(ctx, name):
    """The full frame's mask, rects and records with the block test switched off, once per case: what every other setting's full
    frame must equal.  The strips of a setting are compared with that setting's own full frame, and the frustum half of the block
    test (block_corner's tol) acts on both alike - a block wrongly declared outside the frustum would vanish from both."""
    if name not in _FULL:
        mesh = cases.build_mesh(ctx, case_of(name), "no_block_cull")
        try:
            mesh.render()
            recs, rects, vis = mesh.debug_records()
            _FULL[name] = (vis.copy(), rects.copy(), recs.copy())
        finally:
            mesh.dispose()
    return _FULL[name]


def describe(mask, want, strip):
    lost, extra = np.nonzero(want & ~mask)[0], np.nonzero(mask & ~want)[0]
    return f"strip {strip}: {lost.size} splats of the full frame missing (first {lost[:5].tolist()}), {extra.size} too many (first {extra[:5].tolist()})"


@pytest.mark.parametrize("setting", list(cases.SETTINGS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_strip_is_the_full_frame_cut_at_its_rows(ctx, name, setting):
    """Mask, rects, record rows and stats.visible_splats of every strip against strip_planes of the full frame; the full frame
    itself against the one drawn with the block test switched off (bit-equal: the culls only drop what the exact test drops);
    and the case does what it is for: in some strip at least 50 splats are kept whose centre (the record's cy) lies more than 4 px outside it, and
    the model of the block test, fed the device's own boxes, declares at least 4 blocks dead in some strip (none where the block
    strip test must stand down)."""
    case = case_of(name)
    mesh = cases.build_mesh(ctx, case, setting)
    try:
        _, stats = mesh.render()
        recs, rects, vis = mesh.debug_records()
        assert int(stats.visible_splats) == int(vis.sum()) > 500
        if setting != "no_block_cull":
            b_vis, b_rects, b_recs = full_frame_without_block_cull(ctx, name)
            assert np.array_equal(vis, b_vis), describe(vis, b_vis, "full frame, against the block test switched off")
            assert np.array_equal(rects, b_rects) and np.array_equal(recs, b_recs)
        _, boxes, _ = mesh.debug_cull_planes()
        u = cases.model_uniforms(case)
        cy = recs.view(np.float32)[:, 1].astype(np.float64)
        outside_kept, dead = 0, 0
        for strip in cases.STRIPS:
            _, st = mesh.render(tile_rows=strip)
            s_recs, s_rects, s_vis = mesh.debug_records()
            mask, want_rects, want_recs = ref.strip_planes(vis, rects, recs, *strip)
            assert np.array_equal(s_vis, mask), describe(s_vis, mask, strip)
            assert np.array_equal(s_rects, want_rects), f"strip {strip}: rects differ at {np.nonzero((s_rects != want_rects).any(axis=1))[0][:5].tolist()}"
            assert np.array_equal(s_recs, want_recs), f"strip {strip}: records differ at {np.nonzero((s_recs != want_recs).any(axis=1))[0][:5].tolist()}"
            assert int(st.visible_splats) == int(mask.sum())
            y0, y1 = strip[0] * ref.TILE, min(strip[1] * ref.TILE, cases.H)
            outside_kept = max(outside_kept, int((mask & ((cy < y0 - 4.0) | (cy > y1 + 4.0))).sum()))
            dead = max(dead, int(ref.block_dead(u, boxes, *strip)[1].sum()))
        # These two counts say that the case exercises the culls, not that the device culled: `dead` is the fp64 model's verdict on
        # the device's boxes (the device's own per-block verdict is not read back), taken as the largest over the strips.
        assert outside_kept >= 50, outside_kept
        assert (dead >= 4) if case.block_strip else (dead == 0), dead
    finally:
        mesh.dispose()


@pytest.mark.parametrize("name", cases.NAMES)
def test_upload_planes_behind_the_culls(ctx, name):
    """cov_bound: at least the fp64 spectral radius of the values the shader reads (halves widened) and at most sqrt(3) * 1.0001
    times it - the infinity norm of a symmetric matrix lies between 1 and sqrt(3) times its 2-norm, and the kernel multiplies it by
    1.00001 in fp32 - NaN in, NaN out.  block_box: exactly the min / max of the member centres (NaN left out per coordinate) and
    the largest member bound, NaN if any member's is NaN - also after the case's re-upload."""
    case = case_of(name)
    mesh = cases.build_mesh(ctx, case)
    try:
        bound, boxes, pos = mesh.debug_cull_planes()
    finally:
        mesh.dispose()
    n = case.count
    assert np.array_equal(np.sort(pos), np.arange(n, dtype=np.uint32))                  # a permutation of the storage
    cov = cases.cov_read(case).astype(np.float64)
    finite = np.isfinite(cov).all(axis=1)
    assert np.isnan(bound[np.isnan(cov).any(axis=1)]).all() and not np.isnan(bound[~np.isnan(cov).any(axis=1)]).any()
    assert np.isinf(bound[np.isinf(cov).any(axis=1) & ~np.isnan(cov).any(axis=1)]).all()
    c = cov[finite]
    sym = np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], axis=1).reshape(-1, 3, 3)
    rho = np.abs(np.linalg.eigvalsh(sym)).max(axis=1)
    assert finite.sum() > n - 100 and (bound[finite] >= rho).all() and (bound[finite] <= np.sqrt(3.0) * 1.0001 * rho).all()
    want = ref.block_boxes(cases.final_centers(case), bound, pos, (n + 255) // 256)
    assert np.array_equal(boxes[:, :7], want[:, :7], equal_nan=True), np.nonzero(~((boxes[:, :7] == want[:, :7]) | (np.isnan(boxes[:, :7]) & np.isnan(want[:, :7]))).all(axis=1))[0]
    if name == "straddle":                                                               # the first upload is storage block 0
        assert np.array_equal(np.sort(pos[:256]), np.arange(256)) and boxes[0, 2] < cases.EYE[2] < boxes[0, 5]
    if name == "reupload":                                                               # the moved splats kept their storage positions
        lo, hi, moved = case.reupload
        assert (boxes[np.unique(pos[lo:hi] // 256), 1] <= moved[:, 1].max()).all() and moved[:, 1].max() < 0


@pytest.mark.parametrize("front", ["stream", "compact"])
def test_strips_through_the_visibility_culled_sort(front):
    """The same contract through gs_mesh_project and a visibility-culled sort, for two cases: the sorter's keep bits are the
    expected mask and the sorted list is the pinned sort oracle's order restricted to it.  $GSPLAT_VIS_FRONT is read once per
    process, so each front end gets a child process (tests/tools/strip_cull_sorter.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "strip_cull_sorter.py")], text=True, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, GSPLAT_VIS_FRONT=front))
    tail = [l for l in p.stdout.splitlines() if l.startswith(("FAIL", "strip_cull_sorter"))]
    assert p.returncode == 0 and tail and " 0 failures" in tail[-1] and f"front={front}" in tail[-1], "\n".join(tail[-12:]) or p.stdout[-2000:]
