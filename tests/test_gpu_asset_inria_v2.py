"""-m gpu: the device decode of INRIA-v2 codebook PLY assets (InriaV2Source of csrc/asset_decode.hip: the file's index rows at their own
stride read with byte loads, the decoded codebook copied into LDS by every workgroup) against the host path (gs_asset_fill over the
level-0 image the host builds from the same rows and the same decoded codebook -> gs_mesh_upload, util centres ->
gs_sorter_upload_centers).  Both sides call one row arithmetic (csrc/asset_internal.hpp), and the host reader is pinned bit for bit to
the reference's INRIAV2PlyParser (tests/test_assets_inria_v2_ref.py), so the comparison is np.array_equal - no tolerance - on what
tests/test_gpu_asset_upload.py compares: the sorted index list, distances, the debug planes and one small frame.  That file's helpers
are imported.

The files are small (600 splats: three workgroups, the last partial): what can go wrong here is the partial workgroup (its spare
threads must still copy the codebook and meet the barrier), the byte phase of a row (strides 17 / 26 / 30 / 41 / 62 from any `first`),
the padding behind the last row and the range bookkeeping, and none of those needs a large file."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import asset_inria_v2_cases as VC
import test_gpu_asset_upload as U
from gaussiansplats3d_amd import Context, SplatMesh, assets, create_sort_worker
from gaussiansplats3d_amd import _lib as L
from test_gpu_asset_spz import both

pytestmark = pytest.mark.gpu
N = 600
SH_C0 = 0.28209479177387814
PERMUTED = ["rot_2", "f_rest_4", "x", "opacity", "f_dc_1", "pad", "scale_0", "f_rest_0", "z", "rot_0", "f_rest_8", "f_dc_0", "scale_2",
            "f_rest_1", "f_rest_5", "y", "rot_3", "f_rest_2", "f_dc_2", "f_rest_6", "scale_1", "f_rest_3", "rot_1", "f_rest_7"]
# f_rest fields, bytes per row, writer options
KINDS = {"sh0": (0, 17, {}), "sh1": (9, 26, {}), "sh2": (24, 41, {}), "sh3": (45, 62, {}),
         "sh1_permuted": (9, 30, dict(codebook_first=True, half_type="ushort", comment="x", extra_vertex=[("float", "pad")],
                                      extra_codebook=[("short", "spare")], field_order=PERMUTED))}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_FILES = {}


def synthetic_file(kind, n=N, seed=51):
    """INRIA-v2 bytes of seeded splats laid out for the shared camera, through the package's writer."""
    key = (kind, n, seed)
    if key not in _FILES:
        ncoef, stride, options = KINDS[kind]
        c, s, q, rgba, _ = U.synthetic_splats(n, 0, seed)
        rng = np.random.default_rng(seed + 1)
        sh = rng.normal(0.0, 0.3, size=(n, ncoef)) if ncoef else None
        alpha = np.clip(rgba[:, 3] / 255.0, 0.02, 0.98)
        data = assets.write_inria_v2_ply(c, np.log(s), q, (rgba[:, :3] / 255.0 - 0.5) / SH_C0, np.log(alpha / (1 - alpha)), sh, **options)
        end = data.index(b"end_header\n") + 11
        assert len(data) == end + stride * n + 256 * 2 * (5 + ncoef // 3 + len(options.get("extra_codebook", ()))), "the row is not the stride this kind is for"
        _FILES[key] = data
    return _FILES[key]


def compare_plans(ctx, data, degree, n, plans, tag, transform=None):
    """plans: per pair a list of (path, frm, first, count) into a mesh + sorter of n splats; every pair must show what the first shows."""
    asset = assets.SplatAsset(data, "ply", degree)
    if transform is not None:
        asset.set_transform(transform)
    pairs = [U.Pair(ctx, asset, n, False, True, False, 1) for _ in plans]
    try:
        seen = []
        for pair, plan in zip(pairs, plans):
            for path, frm, first, count in plan:
                (pair.host if path == "host" else pair.device)(frm, first, count)
            seen.append(pair.observe())
        for k in range(1, len(seen)):
            U.assert_same(seen[0], seen[k], f"{tag} plan {k}")
        return seen[0]
    finally:
        for pair in pairs:
            pair.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ reference-checked files
@pytest.mark.parametrize("minimum_alpha", [1, 40])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", VC.cases())
def test_golden_cases(ctx, name, half, minimum_alpha):
    """Every read of tests/golden/assets_inria_v2_ref.npz, whole: both element orders, every file degree at its output degrees, the file
    without scale / colour / opacity fields (alpha 0: nothing is drawn), the hostile codebook.  Integer centres with fp32 covariances,
    float centres with fp16."""
    data, fmt, degree, _ = VC.case(name)
    U.compare_whole(ctx, data, fmt, degree, half, integer=not half, keep_order=False, minimum_alpha=minimum_alpha,
                    expect_pixels=not name.startswith("v2_bare"))


@pytest.mark.parametrize("integer", [True, False])
def test_hostile_centres_through_both_sorters(ctx, integer):
    """NaN / infinite centre halves become INT32_MIN in an integer sorter's message and stay as they are in a float sorter's."""
    data, fmt, degree, _ = VC.case("v2_hostile_d2")
    a = assets.SplatAsset(data, fmt, degree)
    with np.errstate(all="ignore"):
        c = a.fill()["centers"]
    a.close()
    assert np.isnan(c).any() and np.isinf(c).any(), "the hostile halves did not reach the decoded centres"
    U.compare_whole(ctx, data, fmt, degree, half=False, integer=integer, keep_order=False, minimum_alpha=1)


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("count", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("kind", ["sh3", "sh0"])
def test_counts(ctx, kind, count):
    """One lane, one lane short of a workgroup, exactly one, one more, two and one more: the partial last workgroup still loads the codebook."""
    seen = compare_plans(ctx, synthetic_file(kind), 2, count, both([(0, 0, count)]), f"{kind} count {count}")
    assert count < 255 or (seen["frame"].any() and seen["visible"].any())


# ------------------------------------------------------------------------------------------------ ranges
@pytest.mark.parametrize("first", [1, 2, 3, 255, 257])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_first_at_every_byte_phase(ctx, kind, first):
    """The file rotated by `first` splats: the staged rows start at byte stride * first of the file's element but at the aligned staging
    base on the device, and the second piece has from != 0 with first = 0."""
    seen = compare_plans(ctx, synthetic_file(kind), 2, N, both([(0, first, N - first), (N - first, 0, first)]), f"{kind} first {first}")
    assert seen["frame"].any() and seen["visible"].any()


@pytest.mark.parametrize("kind", ["sh0", "sh2", "sh1_permuted"])
def test_pieces_out_of_order_and_mixed_paths(ctx, kind):
    moves = [(300, 300, 300), (0, 0, 255), (255, 255, 45)]                  # the tail first, then two unequal pieces
    plans = both(moves) + [[("host", *moves[0]), ("device", *moves[1]), ("host", *moves[2])],
                           [("device", *moves[0]), ("host", *moves[1]), ("device", *moves[2])],
                           [("host", 0, 0, N)]]
    compare_plans(ctx, synthetic_file(kind), 2, N, plans, kind)


@pytest.mark.parametrize("kind", ["sh3", "sh0"])
def test_padding_is_never_part_of_a_value(kind, monkeypatch):
    """Under GSPLAT_POISON_ALLOC=0xFF the staging buffer's padding behind the last row holds 0xFF instead of zeros: ranges whose rows end
    at every byte phase decode to what the host path shows."""
    monkeypatch.setenv("GSPLAT_POISON_ALLOC", "0xFF")                    # (read at every allocation: stays set for the whole test)
    pctx = Context(0)
    try:
        for first, count in ((0, 1), (3, 2), (1, 255), (2, 257), (257, 343)):
            compare_plans(pctx, synthetic_file(kind), 2, count, both([(0, first, count)]), f"{kind} poisoned {first}+{count}")
    finally:
        pctx.close()


# ------------------------------------------------------------------------------------------------ degrees, transforms
@pytest.mark.parametrize("degree", [2, 1, 0])
def test_degree_3_file_into_a_smaller_mesh(ctx, degree):
    """A degree-3 file's rows are staged whole (62 bytes per splat); only the fields and the codebook pages of the bands the mesh keeps
    are read."""
    data = synthetic_file("sh3")
    a = assets.SplatAsset(data, "ply", degree)
    assert (a.info.splat_count, a.info.sh_degree) == (N, degree)
    a.close()
    compare_plans(ctx, data, degree, N, both([(0, 0, N)]), f"degree {degree}")


@pytest.mark.parametrize("kind", ["sh2", "sh1_permuted"])
def test_transformed(ctx, kind):
    """A non-uniform scale, a small rotation and a translation baked on both paths, both kernels (the scene stays in view)."""
    ang = 0.05
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    m = np.eye(4)
    m[:3, :3] = rot @ np.diag([1.1, 0.9, 1.05])
    m[:3, 3] = [0.1, -0.05, 0.02]
    data = synthetic_file(kind)
    moved = compare_plans(ctx, data, 2, N, both([(0, 3, N - 3), (N - 3, 0, 3)]), kind, transform=m.T.reshape(-1))
    plain = compare_plans(ctx, data, 2, N, both([(0, 3, N - 3), (N - 3, 0, 3)]), kind)
    assert moved["frame"].any() and not np.array_equal(moved["distances"], plain["distances"]), "the transform moved nothing"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(ctx):
    data1 = synthetic_file("sh1")
    asset1, asset_deg0 = assets.SplatAsset(data1, "ply", 1), assets.SplatAsset(data1, "ply", 0)
    pair = U.Pair(ctx, asset1, N, False, True, False, 1)                            # a half-SH mesh of degree 1
    dynamic = create_sort_worker(ctx, N, integer_based_sort=True, dynamic_mode=True)
    try:
        pair.device(0, 0, N)
        before = pair.observe()
        assert before["frame"].any()

        def refused(call):
            with pytest.raises(L.GsError) as e:
                call()
            assert e.value.status == L.GS_ERR_INVALID

        refused(lambda: asset_deg0.upload_to(pair.mesh, 0, 0, N))                   # read at degree 0 into a degree 1 mesh
        refused(lambda: asset1.upload_to(pair.mesh, 0, N - 10, 11))                 # first + count leaves the asset
        refused(lambda: asset1.upload_to(pair.mesh, N - 10, 0, 11))                 # from + count leaves the mesh
        refused(lambda: asset1.upload_centers_to(pair.worker, 0, N - 10, 11))
        refused(lambda: asset1.upload_centers_to(pair.worker, N - 10, 0, 11))
        mesh8 = SplatMesh(ctx, N, 1, spherical_harmonics_8bit=True)
        refused(lambda: asset1.upload_to(mesh8, 0, 0, N))                           # half SH (sh_level 1) into a GS_MESH_SH_U8 mesh
        mesh8.dispose()
        asset_deg0.set_transform(np.diag([2.0, 2.0, 2.0, 1.0]).reshape(-1))         # a dynamic sorter takes no baked transform
        refused(lambda: asset_deg0.upload_centers_to(dynamic, 0, 0, N, scene_indexes=np.zeros(N, np.uint32)))
        asset_deg0.set_transform(None)
        asset_deg0.upload_centers_to(dynamic, 0, 0, N, scene_indexes=np.zeros(N, np.uint32))
        U.assert_same(before, pair.observe(), "after the refused calls")
    finally:
        dynamic.terminate()
        pair.close()
        asset1.close()
        asset_deg0.close()


# ------------------------------------------------------------------------------------------------ Node
def test_round_trip_through_node(ctx, tmp_path):
    """node/asset_formats_via_js.js opens the .ply by name (the library decides the flavour from the header), uploads it through the
    device decode and draws what the Python mirror draws."""
    assert shutil.which("node") is not None, "node is not installed"
    subprocess.check_call(["make", "-C", U.NODE_DIR], stdout=subprocess.DEVNULL)
    data, degree = synthetic_file("sh3"), 2
    asset = assets.SplatAsset(data, None, degree)
    pair = U.Pair(ctx, asset, N, False, True, False, 1)
    try:
        pair.device(0, 0, N)
        seen = pair.observe()
    finally:
        pair.close()
        asset.close()
    fpath, ipath, opath = str(tmp_path / "a.ply"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fpath, "wb").write(data)
    cam = U.CAM
    fx, fy = cam.focal()
    with open(ipath, "wb") as f:
        for p in (np.array([U.W, U.H, degree, 0], np.uint32), np.asarray(cam.model_view(), np.float64).astype(np.float32),
                  np.asarray(cam.projection, np.float64).astype(np.float32), np.asarray(cam.position, np.float32),
                  np.array([fx, fy], np.float32), np.asarray(cam.sort_mvp(), np.float64).astype(np.float32)):
            f.write(np.ascontiguousarray(p).tobytes())
    res = subprocess.run(["node", "asset_formats_via_js.js", fpath, ipath, opath], cwd=U.NODE_DIR, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["splatCount"] == N and info["format"] == L.GS_ASSET_PLY and info["shDegree"] == 2
    raw = np.fromfile(opath, dtype=np.uint8)
    assert np.array_equal(raw[:4 * N].view(np.uint32), seen["order"]), "sorterUploadAssetCenters + sort differs from the Python mirror"
    frame = raw[4 * N:].reshape(U.H, U.W, 4)
    assert frame.any() and np.array_equal(frame, seen["frame"]), "meshUploadAsset + draw differs from the Python mirror"
