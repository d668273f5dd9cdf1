"""-m gpu: the device decode of an asset WITH a static scene transform (gs_asset_set_transform, then gs_mesh_upload_asset /
gs_sorter_upload_asset_centers: the XF instantiations of csrc/asset_decode.hip) against the host path of the same transformed
asset (gs_asset_fill -> gs_mesh_upload [+ gs_mesh_upload_sh_u8], util.integer_centers / float_centers ->
gs_sorter_upload_centers).  The host fill is pinned bit for bit to the reference's transformed fills
(tests/test_assets_transform_ref.py), so "device == host, bit for bit" pins the device path to the reference too.

The method is tests/test_gpu_asset_upload.py's: mesh + sorter A through the host path, B through the device calls, and
np.array_equal - no tolerance - on the sorted order, the frame, gs_mesh_compute_distances and the per-splat records, rects and
visibility.  The camera is per case (tests/asset_transform_cases.py): it looks at the transformed cluster of the golden files,
and every case requires a frame that is not empty and at least a quarter of the splats visible."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import asset_transform_cases as K
import test_gpu_asset_upload as base
from gaussiansplats3d_amd import Context, SplatMesh, assets, create_sort_worker
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


class Pair:
    """One mesh + one sorter of n splats, filled range by range from (transformed) assets, and what a sort + draw shows."""

    def __init__(self, ctx, info, n, cam, half=False, integer=True, keep_order=False, minimum_alpha=1):
        self.n, self.cam, self.half, self.min_alpha = n, cam, half, minimum_alpha
        self.mesh = SplatMesh(ctx, n, info.sh_degree, half_precision_covariances=half,
                              spherical_harmonics_8bit=info.sh_level == 2 and info.sh_degree > 0, keep_order=keep_order)
        if self.mesh.sh_8bit:
            self.mesh.set_scenes(sh8_range=[(info.sh_min, info.sh_max)])
        self.worker = create_sort_worker(ctx, n, integer_based_sort=integer)

    def host(self, asset, frm, first, count):
        with np.errstate(all="ignore"):
            filled = asset.fill(self.min_alpha, self.half)
            base.host_upload(self.mesh, filled, frm, first, count)
            base.host_centers(self.worker, filled, frm, first, count)

    def device(self, asset, frm, first, count):
        asset.upload_to(self.mesh, frm, first, count, self.min_alpha)
        asset.upload_centers_to(self.worker, frm, first, count)

    def observe(self):
        n, cam = self.n, self.cam
        reply = self.worker.post_message({"sort": {"modelViewProj": cam.sort_mvp(), "splatRenderCount": n, "splatSortCount": n}})
        order = reply["sortedIndexes"].copy()
        self.mesh.set_camera(cam)
        self.mesh.update_render_indexes(order, n)
        frame, _ = self.mesh.render()
        recs, rects, vis = self.mesh.debug_records(n)
        dist = np.empty(n, np.int32)
        self.mesh.compute_distances_on_gpu(cam.sort_mvp(), out=dist, integer=True)
        return {"order": order, "frame": frame, "records": recs, "rects": rects, "visible": vis, "distances": dist}

    def close(self):
        self.worker.terminate()
        self.mesh.dispose()


def assert_seen(o, tag=""):
    """Equal empty frames would prove nothing."""
    share = float(o["visible"].mean())
    assert o["frame"].any(), f"{tag}: the frame is empty"
    assert share >= K.MIN_IN_VIEW, f"{tag}: only {share:.3f} of the splats are visible"


def compare(ctx, plans, info, n, cam, tag="", **kw):
    """plans: per pair a list of (path, asset, frm, first, count); every pair must show what the first shows."""
    pairs = [Pair(ctx, info, n, cam, **kw) for _ in plans]
    try:
        seen = []
        for pair, plan in zip(pairs, plans):
            for path, asset, frm, first, count in plan:
                (pair.host if path == "host" else pair.device)(asset, frm, first, count)
            seen.append(pair.observe())
        assert_seen(seen[0], tag)
        for k in range(1, len(seen)):
            base.assert_same(seen[0], seen[k], f"{tag} plan {k}")
        return seen[0]
    finally:
        for pair in pairs:
            pair.close()


def transformed_centers(asset):
    with np.errstate(all="ignore"):
        return asset.fill()["centers"]


# ------------------------------------------------------------------------------------------------ reference-written files
GOLDEN_CASES = [(case, tag, name, half) for case in K.CASES for tag in K.TAGS for name in K.TRANSFORMS for half in (False, True)]


@pytest.mark.parametrize("k", range(len(GOLDEN_CASES)), ids=["-".join(map(str, c)) for c in GOLDEN_CASES])
def test_reference_written_files_with_a_transform(ctx, k):
    """Every golden file (150 to 420 splats: a partial last workgroup) x the five transforms x both covariance precisions; integer
    / float sorters and keep_order alternate over the cases."""
    case, tag, name, half = GOLDEN_CASES[k]
    integer, keep_order = k % 2 == 0, (k // 2) % 3 == 0
    data, fmt, deg = K.file_of(case, tag)
    asset = assets.SplatAsset(data, fmt, deg)
    try:
        asset.set_transform(K.matrix(name))
        n = asset.info.splat_count
        compare(ctx, [[("host", asset, 0, 0, n)], [("device", asset, 0, 0, n)]], asset.info, n, K.golden_camera(name),
                f"{case} {tag} {name}", half=half, integer=integer, keep_order=keep_order)
    finally:
        asset.close()


# ------------------------------------------------------------------------------------------------ larger synthetic files
def synthetic(level, sh_degree, n=24_000):
    data = base.synthetic_file(n, level, sh_degree, block_size=4.0, bucket_size=128, seed=9)
    hd = base.ksplat_header(data)
    assert hd["level"] == level and hd["splats"] == n
    assert hd["full"] >= 8 and hd["partial"] >= 2, hd                    # both bucket paths are taken
    return data


@pytest.mark.parametrize("level,sh_degree", [(2, 2), (1, 1)])
def test_larger_file_in_three_unequal_pieces_with_first_differing_from_from(ctx, level, sh_degree):
    n = 24_000
    asset = assets.SplatAsset(synthetic(level, sh_degree, n), "ksplat", sh_degree)
    try:
        asset.set_transform(K.matrix("nonuniform"))
        moves = [(100, 0, 5_001), (5_101, 5_001, n - 100 - 5_001), (0, n - 100, 100)]       # the file rotated by 100 splats
        assert all(frm != first for frm, first, _ in moves) and sum(c for _, _, c in moves) == n
        compare(ctx, [[("host", asset, *m) for m in moves], [("device", asset, *m) for m in moves]], asset.info, n,
                K.cloud_camera(transformed_centers(asset)), f"level {level}", half=level == 2, integer=sh_degree != 1)
    finally:
        asset.close()


# ------------------------------------------------------------------------------------------------ two scenes in one mesh
def test_two_scenes_with_their_own_transforms_in_one_mesh(ctx):
    """addSplatScenes in static mode: asset 1 with `rigid` -> [0, n1), asset 2 with `mirror` -> [n1, n1 + n2); also in the
    opposite call order."""
    a1 = assets.SplatAsset(*K.file_of("sh2", "gen1"))
    a2 = assets.SplatAsset(*K.file_of("sh2", "gen0"))
    try:
        a1.set_transform(K.matrix("rigid"))
        a2.set_transform(K.matrix("mirror"))
        n1, n2 = a1.info.splat_count, a2.info.splat_count
        assert a1.info.sh_degree == a2.info.sh_degree == 2 and a1.info.sh_level == a2.info.sh_level == 1
        cam = K.cloud_camera(np.concatenate([transformed_centers(a1), transformed_centers(a2)]))
        one, two = (a1, 0, 0, n1), (a2, n1, 0, n2)
        compare(ctx, [[("host", *one), ("host", *two)], [("device", *one), ("device", *two)], [("device", *two), ("device", *one)]],
                a1.info, n1 + n2, cam, "two scenes")
    finally:
        a1.close()
        a2.close()


# ------------------------------------------------------------------------------------------------ hostile rows
@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("half", [False, True])
def test_hostile_rows_under_a_transform(ctx, half, integer):
    """NaN / infinite centres, a NaN scale and an infinite SH coefficient through the `uniform` transform."""
    asset = assets.SplatAsset(base._hostile_level0(), "ksplat", 1)
    try:
        asset.set_transform(K.matrix("uniform"))
        c = transformed_centers(asset)
        assert np.isnan(c).any(), "the hostile centres did not reach the transformed arrays"
        n = asset.info.splat_count
        compare(ctx, [[("host", asset, 0, 0, n)], [("device", asset, 0, 0, n)]], asset.info, n, K.cloud_camera(c), "hostile",
                half=half, integer=integer)
    finally:
        asset.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(ctx):
    n = 24_000
    asset = assets.SplatAsset(synthetic(1, 1, n), "ksplat", 1)
    asset.set_transform(K.matrix("rigid"))
    cam = K.cloud_camera(transformed_centers(asset))
    pair = Pair(ctx, asset.info, n, cam)
    dynamic = create_sort_worker(ctx, n, dynamic_mode=True)
    scene = np.zeros(n, np.uint32)
    sort = {"sort": {"modelViewProj": cam.sort_mvp(), "splatRenderCount": n, "splatSortCount": n,
                     "transforms": np.eye(4, dtype=np.float32).reshape(16)}}
    try:
        pair.device(asset, 0, 0, n)
        before = pair.observe()
        assert_seen(before, "before")
        asset.set_transform(None)                                        # a dynamic sorter takes the untransformed centres ...
        asset.upload_centers_to(dynamic, 0, 0, n, scene_indexes=scene)
        order_before = dynamic.post_message(sort)["sortedIndexes"].copy()
        asset.set_transform(K.matrix("rigid"))

        def refused(call):
            with pytest.raises(L.GsError) as e:
                call()
            assert e.value.status == L.GS_ERR_INVALID

        refused(lambda: asset.upload_centers_to(dynamic, 0, 0, n, scene_indexes=scene))   # ... and refuses baked ones
        assert np.array_equal(dynamic.post_message(sort)["sortedIndexes"], order_before)
        bad = K.matrix("rigid")
        bad[7] = 0.5                                                     # a projective bottom row
        refused(lambda: asset.set_transform(bad))
        bad = K.matrix("rigid")
        bad[13] = np.nan
        refused(lambda: asset.set_transform(bad))
        again = Pair(ctx, asset.info, n, cam)                            # the asset kept `rigid`: a fresh upload shows the same
        try:
            again.device(asset, 0, 0, n)
            base.assert_same(before, again.observe(), "after the refused matrices")
        finally:
            again.close()
        base.assert_same(before, pair.observe(), "after the refused calls")
    finally:
        dynamic.terminate()
        pair.close()
        asset.close()


# ------------------------------------------------------------------------------------------------ Node
def test_transformed_upload_through_node_matches_the_python_mirror(ctx, tmp_path):
    """buildFromAsset / uploadAssetCenters with a trailing transform through node/gsplat.js: the order and the frame of the
    level-2 synthetic file under `uniform` equal the Python mirror's."""
    assert shutil.which("node") is not None, "node is not installed"
    subprocess.check_call(["make", "-C", base.NODE_DIR], stdout=subprocess.DEVNULL)
    n = 24_000
    data = synthetic(2, 1, n)
    m = K.matrix("uniform")
    asset = assets.SplatAsset(data, "ksplat", 1)
    try:
        asset.set_transform(m)
        cam = K.cloud_camera(transformed_centers(asset))
        seen = compare(ctx, [[("device", asset, 0, 0, n)]], asset.info, n, cam, "python mirror")
    finally:
        asset.close()
    fpath, ipath, opath = str(tmp_path / "a.ksplat"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fpath, "wb").write(data)
    fx, fy = cam.focal()
    with open(ipath, "wb") as f:
        for p in (np.array([K.W, K.H, 1, 1], np.uint32), np.asarray(cam.model_view(), np.float64).astype(np.float32),
                  np.asarray(cam.projection, np.float64).astype(np.float32), np.asarray(cam.position, np.float32),
                  np.array([fx, fy], np.float32), np.asarray(cam.sort_mvp(), np.float64).astype(np.float32), np.asarray(m, np.float64)):
            f.write(np.ascontiguousarray(p).tobytes())
    res = subprocess.run(["node", "asset_transform_via_js.js", fpath, ipath, opath], cwd=base.NODE_DIR, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["splatCount"] == n and info["uploaded"] == n
    raw = np.fromfile(opath, dtype=np.uint8)
    order = raw[:4 * n].view(np.uint32)
    frame = raw[4 * n:].reshape(K.H, K.W, 4)
    assert np.array_equal(order, seen["order"]), "uploadAssetCenters with a transform + sort differs from the Python mirror"
    assert frame.any() and np.array_equal(frame, seen["frame"]), "buildFromAsset with a transform + draw differs from the Python mirror"
