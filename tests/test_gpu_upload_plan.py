"""-m gpu: one mesh of 1000 splats (three storage blocks and a part of a fourth) filled by five uploads that cut one call up to
four times, leave gaps of never-uploaded splats, touch and overlap - the upload's host policy (csrc/upload_plan.cpp) as the
device shows it.  After every upload the storage position of every splat, every block box and every covariance bound are read
back and held to the host models: upload_plan_ref (which segments are fresh), strip_cull_cases.morton_positions (the slots a
fresh segment receives), strip_cull_ref.block_boxes (over the centres the mesh now holds - also for blocks an upload touched only
through the range that held its splats) and bounds_ref."""
import numpy as np
import pytest

import bounds_ref
import strip_cull_cases as cases
import strip_cull_ref
import upload_plan_ref as ref
from gaussiansplats3d_amd import Context, GsError, SplatMesh
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
N = 1000
BLOCKS = (N + 255) // 256
STEPS = [(100, 300), (500, 700), (0, 600), (700, 1000), (650, 750)]
CENTER = (0.3, -1.7, 2.9)
SH_COEFS = 9


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def cov_bound_f32(cov):
    """cov_spectral_bound of mesh.hip as the device evaluates it: fp32 sums left to right, the largest, times 1.00001f."""
    a = np.abs(np.asarray(cov, np.float32).reshape(-1, 6))
    r = np.stack([(a[:, 0] + a[:, 1]) + a[:, 2], (a[:, 1] + a[:, 3]) + a[:, 4], (a[:, 2] + a[:, 4]) + a[:, 5]], axis=1)
    return (r.max(axis=1) * np.float32(1.00001)).astype(np.float32)


def step_data(k):
    """What upload k carries: random centres in a box (NaN centres in the fresh middle segment of the third upload; the fifth
    mirrors what the mesh holds through a plane far away), covariances, colours and 8-bit SH."""
    a, b = STEPS[k]
    rng = np.random.default_rng(4000 + k)
    c = cases.slab(rng, b - a)
    if k == 2:
        c[310 - a] = np.nan
        c[311 - a] = np.nan
        c[450 - a, 1] = np.nan
    return c, cases.blobs(rng, b - a), cases.colours(rng, b - a), rng.integers(0, 256, size=(b - a, SH_COEFS), dtype=np.uint8)


def read_planes(mesh):
    """(cov_bound, position) of the splats below the mesh's uploaded count, and every block box of the mesh."""
    n = mesh.splat_count
    bound, pos, boxes = np.empty(n, np.float32), np.empty(n, np.uint32), np.empty((BLOCKS, 8), np.float32)
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 10, bound.ctypes.data, n))
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 11, boxes.ctypes.data, BLOCKS))
    L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 12, pos.ctypes.data, n))
    return bound, boxes, pos


def side_uploads(mesh, start, count):
    """(status, message) of an 8-bit-SH upload and of a scene-index upload for [start, start + count)."""
    sh = np.full((count, SH_COEFS), 128, np.uint8)
    idx = np.zeros(count, np.uint32)
    out = []
    for fn, arr in ((mesh.lib.gs_mesh_upload_sh_u8, sh), (mesh.lib.gs_mesh_upload_scene_indexes, idx)):
        st = fn(mesh.handle, start, count, arr.ctypes.data)
        out.append((st, mesh.lib.gs_last_error().decode() if st < 0 else ""))
    return out


def same_bounds(got, want):
    assert got["count"] == want["count"], (got, want)
    assert got["min"].tobytes() == np.asarray(want["min"], np.float32).tobytes(), (got, want)
    assert got["max"].tobytes() == np.asarray(want["max"], np.float32).tobytes(), (got, want)
    assert np.float64(got["max_dist_sq"]).tobytes() == np.float64(want["max_dist_sq"]).tobytes(), (got, want)


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
def test_five_uploads_against_the_models(ctx, keep_order):
    mesh = SplatMesh(ctx, N, 1, spherical_harmonics_8bit=True, keep_order=keep_order)
    centres, cov = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32)     # what a never-uploaded splat holds
    pos = np.arange(N, dtype=np.int64)                                             # ... and where it sits
    ranges, cuts = [], []
    try:
        for k, (a, b) in enumerate(STEPS):
            if k == 2:   # [300, 500) owns no slots yet: its SH and scene indexes have nowhere to go - unless the mesh keeps upload order
                for st, msg in side_uploads(mesh, 300, 200):
                    assert (st == 0) if keep_order else (st == L.GS_ERR_INVALID and "upload the splats with gs_mesh_upload before their" in msg), (st, msg)
            c, cv, rgba, sh = step_data(k)
            if k == 4:
                c = centres[a:b].copy()
                c[:, 0] = np.float32(-200.0) - c[:, 0]
            segments = ref.plan_upload(ranges, a, b - a, not keep_order)
            mesh.build(c, cv, rgba, sh, start=a)
            centres[a:b], cov[a:b] = c, cv
            for lo, hi, fresh, _, _ in segments:           # a fresh segment receives the Morton order of the centres it has now
                if fresh and not keep_order:
                    pos[lo:hi] = cases.morton_positions(centres, [(lo, hi)])[lo:hi]
            ranges = ref.ranges_after(ranges, a, b - a)
            cuts.append([s[:3] for s in segments])
            n = mesh.splat_count
            assert n == max(e for _, e in STEPS[:k + 1])
            bound, boxes, got_pos = read_planes(mesh)
            assert np.array_equal(got_pos, pos[:n]), (k, np.nonzero(got_pos != pos[:n])[0][:8])
            assert np.array_equal(np.sort(pos), np.arange(N))                      # with the identity beyond `uploaded`: a bijection
            want_bound = cov_bound_f32(cov)
            assert np.array_equal(bound, want_bound[:n]), k
            assert np.allclose(want_bound, strip_cull_ref.cov_bound(cov), rtol=5 * 2.0 ** -24, atol=0)     # the model's, within the four fp32 roundings
            want = strip_cull_ref.block_boxes(centres, want_bound, pos, BLOCKS)
            assert np.array_equal(boxes[:, :7], want[:, :7], equal_nan=True), (k, np.nonzero((boxes[:, :7] != want[:, :7]).any(axis=1))[0])
        fresh = 1 if keep_order else 0
        assert cuts[2] == [(0, 100, 1), (100, 300, fresh), (300, 500, 1), (500, 600, fresh)] and cuts[4] == [(650, 750, fresh)]
        assert ranges == [(0, N)]
        if not keep_order:                                 # the mirrored splats kept their slots, all over the storage
            assert np.unique(pos[650:750] // 256).size >= 2 and not np.array_equal(pos, np.arange(N))
            assert (boxes[:, 0] < -190.0).sum() >= 2       # ... and every block that holds one has a box that reaches them
        else:
            assert np.array_equal(pos, np.arange(N))
        for st, msg in side_uploads(mesh, 300, 200):
            assert st == 0, (st, msg)
        for start, count in [(650, 100), (0, N)]:
            same_bounds(mesh.bounds(start, count, CENTER), bounds_ref.bounds(centres, CENTER, start, count))
        for start, count in [(900, 101), (N, 1), (0xFFFFFFF0, 0x20)]:
            with pytest.raises(GsError, match="the range is not wholly uploaded"):
                mesh.bounds(start, count, CENTER)
    finally:
        mesh.dispose()
