"""-m gpu: streamed assets on the device (gs_asset_open_stream / gs_asset_append, then gs_mesh_upload_asset and
gs_sorter_upload_asset_centers on the ready prefix; the INRIA-v1 row source of csrc/asset_sources.hpp).

Rule P, per format: one mesh + sorter receives the whole-file asset by a plan of pieces, the other receives the stream by the same
pieces, each uploaded right after the append that made it ready (appends are cut mid-row).  What a sort + draw of the two shows
(test_gpu_asset_upload.Pair.observe: order, distances, visible, rects, records, frame) must be np.array_equal, and the frame must
not be empty.  The INRIA-v1 device source is held to the host image of the whole-file reader the same way.  The CPU half (the
ready prefix against a model, every refusal) is tests/test_asset_stream.py."""
import numpy as np
import pytest

import asset_stream_cases as SC
import ksplat_sections
import test_gpu_asset_upload as U
from gaussiansplats3d_amd import Context, assets
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
N = 24_000
APPEND = 262_144


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_FILES = {}


def big_file(kind):
    """(bytes, fmt, degree to open at): 24 000 seeded splats laid out for the shared camera."""
    if kind in _FILES:
        return _FILES[kind]
    c, s, q, rgba, _ = U.synthetic_splats(N, 0, 61)
    rng = np.random.default_rng(62)
    logit = rng.normal(2.0, 2.0, size=N)
    f_dc = rng.normal(0.5, 1.0, size=(N, 3))
    if kind in ("v1_sh0", "v1_sh2", "v1_odd"):
        n_rest = {"v1_sh0": 0, "v1_sh2": 24, "v1_odd": 9}[kind]
        rest = rng.normal(0, 0.3, size=(N, n_rest)).astype(np.float32) if n_rest else None
        extra = rng.integers(0, 256, N).astype(np.uint8) if kind == "v1_odd" else None
        out = (assets.write_ply(c, np.log(s), q, f_dc, logit, rest, extra), "ply", 0 if kind == "v1_sh0" else 2)
    elif kind == "splat":
        out = (assets.write_splat(c, s, q, rgba), "splat", 0)
    elif kind in ("pc_sh0", "pc_sh2", "pc_sh2_at_0"):
        sh = rng.normal(0.0, 0.4, size=(N, 24)) if kind != "pc_sh0" else None
        out = (assets.write_compressed_ply(c, np.log(s), q, rgba / 255.0, sh), "ply", 0 if kind == "pc_sh2_at_0" else 2)
    elif kind == "ksplat":                                   # two sections of 12 000, level 1, buckets of 128
        halves = [assets.write_ksplat(c[h], s[h], q[h], rgba[h], rng.normal(0, 0.4, size=(N // 2, 9)), 1, 1, block_size=4.0,
                                      bucket_size=128)[0] for h in (slice(0, N // 2), slice(N // 2, N))]
        out = (ksplat_sections.join(halves), "ksplat", 1)
    elif kind == "spz":
        out = (assets.write_spz(c, np.log(s), q, rgba / 255.0, rng.normal(0, 0.4, size=(N, 9))), "spz", 2)
    elif kind == "iv2":
        out = (assets.write_inria_v2_ply(c, np.log(s), q, f_dc, logit, rng.normal(0, 0.3, size=(N, 9))), "ply", 2)
    _FILES[kind] = out
    return out


KINDS = ["v1_sh0", "v1_sh2", "v1_odd", "splat", "pc_sh0", "pc_sh2", "pc_sh2_at_0", "ksplat", "spz", "iv2"]


def pieces(points):
    return [(a, b - a) for a, b in zip(points[:-1], points[1:])]


PLANS = {
    "per_append": None,                                                        # one piece per 262144-byte append
    "1_255_256_257": pieces([0, 1, 256, 512, 769, N]),
    # [511, 513) straddles a compressed-PLY chunk border, [11 990, 12 010) the .ksplat section border
    "straddles": pieces([0, 511, 513, 11_990, 12_010, N]),
}


def run_stream(ctx, kind, plan, append=APPEND):
    data, fmt, degree = big_file(kind)
    whole = assets.SplatAsset(data, fmt, degree)
    stream = assets.SplatAssetStream(fmt, degree, len(data))
    assert whole.info.splat_count == N
    fed = 0

    def feed():
        nonlocal fed
        end = min(fed + append, len(data))
        stream.append(data[fed:end], end == len(data))
        fed = end

    while stream.info is None:                               # a mesh is sized from the header
        feed()
    a, b = (U.Pair(ctx, asset, N, False, True, False, 1) for asset in (whole, stream))
    try:
        if plan is None:
            done = 0
            while True:
                ready = stream.stream_info.splats_ready
                if ready > done:
                    a.device(done, done, ready - done)
                    b.device(done, done, ready - done)
                    done = ready
                if fed == len(data):
                    break
                feed()
            assert done == N
        else:
            for first, count in plan:
                while stream.stream_info.splats_ready < first + count:
                    feed()
                a.device(first, first, count)
                b.device(first, first, count)
            while fed < len(data):
                feed()
        assert stream.stream_info.complete == 1
        oa, ob = a.observe(), b.observe()
        assert oa["frame"].any() and oa["visible"].any(), "the camera sees nothing: the case would compare empty frames"
        U.assert_same(oa, ob, kind)
    finally:
        a.close()
        b.close()
        whole.close()
        stream.close()


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("kind", KINDS)
def test_pieces_of_a_stream_leave_what_the_whole_file_leaves(ctx, kind, plan):
    # 262 144-byte appends cut rows of 68, 248, 105, 32, 16 and 42 bytes in the middle; 100 003 is odd, for the piece plans
    run_stream(ctx, kind, PLANS[plan], APPEND if PLANS[plan] is None else 100_003)


def test_streams_are_ready_early_where_the_format_allows(ctx):
    """The plan above would also pass if everything became ready at the end: here the first append must make splats ready for the
    formats that stream, and none for the two that cannot."""
    for kind, early in (("v1_sh2", True), ("v1_odd", True), ("splat", True), ("pc_sh0", True), ("pc_sh2_at_0", True), ("ksplat", True),
                        ("pc_sh2", False), ("spz", False), ("iv2", False)):
        data, fmt, degree = big_file(kind)
        s = assets.SplatAssetStream(fmt, degree, len(data))
        s.append(data[:APPEND])
        assert (s.stream_info.splats_ready > 0) == early, kind
        s.close()


# ------------------------------------------------------------------------------------------------ the INRIA-v1 device source
_SMALL = {}


def small_v1(name, n):
    if (name, n) not in _SMALL:
        centers = U.synthetic_splats(n, 0, 71)[0]
        _SMALL[(name, n)] = SC.v1_case(name, n, centers)
    return _SMALL[(name, n)]


def transform():
    ang = 0.05
    m = np.eye(4)
    m[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ np.diag([1.1, 0.9, 1.05])
    m[:3, 3] = [0.1, -0.05, 0.02]
    return m.T.reshape(-1)


def completed_stream(data, fmt, degree, step=4093):
    s = assets.SplatAssetStream(fmt, degree, len(data))
    ends = SC.by_size(len(data), step)
    for _ in SC.feed(s, data, ends):
        pass
    return s


def host_image_against_device_source(ctx, name, n, half, integer, minimum_alpha, xf):
    data, fmt, degree = small_v1(name, n)
    whole, stream = assets.SplatAsset(data, fmt, degree), completed_stream(data, fmt, degree)
    assert stream.info.splat_count == n
    if xf:
        whole.set_transform(transform())
        stream.set_transform(transform())
    a, b = (U.Pair(ctx, asset, n, half, integer, False, minimum_alpha) for asset in (whole, stream))
    try:
        a.host(0, 0, n)                                      # gs_asset_fill of parse_ply's image -> gs_mesh_upload
        b.device(0, 0, n)                                    # the file's rows -> k_asset_decode<InriaV1Source>
        oa, ob = a.observe(), b.observe()
        if n > 1 and name != "v1_rgb_no_scale":              # (no opacity field: every splat of that file is transparent)
            assert oa["frame"].any() and oa["visible"].any(), "the camera sees nothing: the case would compare empty frames"
        U.assert_same(oa, ob, name)
    finally:
        a.close()
        b.close()
        whole.close()
        stream.close()


@pytest.mark.parametrize("xf", [False, True])
@pytest.mark.parametrize("minimum_alpha", [1, 40])
@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", sorted(SC.V1_CASES))
def test_inria_v1_device_source_against_the_host_image(ctx, name, half, integer, minimum_alpha, xf):
    host_image_against_device_source(ctx, name, 257, half, integer, minimum_alpha, xf)


@pytest.mark.parametrize("n", [1, 255, 256])
@pytest.mark.parametrize("name", ["v1_sh3", "v1_odd_stride"])
def test_inria_v1_device_source_at_the_workgroup_edges(ctx, name, n):
    host_image_against_device_source(ctx, name, n, False, True, 1, False)


@pytest.mark.parametrize("half", [False, True])
def test_rotation_nans_are_the_same_bits_on_the_host_and_the_device(ctx, half):
    """Rows with an infinite or NaN rot_*: a stream stores the canonical NaN in its level-0 tuple on both sides, so the host fill of
    the completed stream and the device decode of its rows leave the same bits (tests/test_asset_stream.py holds the same file to
    gs_asset_open: NaN in the same places, everything else bit-equal)."""
    data, fmt, degree = small_v1("v1_nan_rotations", 257)
    stream = completed_stream(data, fmt, degree)
    a, b = (U.Pair(ctx, stream, 257, half, True, False, 1) for _ in range(2))
    try:
        with np.errstate(all="ignore"):
            assert np.isnan(a.filled["cov_f16" if half else "cov"].view(np.float16 if half else np.float32)[SC.NAN_ROTATION_ROWS]).all()
        a.host(0, 0, 257)
        b.device(0, 0, 257)
        oa, ob = a.observe(), b.observe()
        assert oa["frame"].any()
        U.assert_same(oa, ob, "v1_nan_rotations")
    finally:
        a.close()
        b.close()
        stream.close()


def test_the_hostile_rows_reach_the_arrays():
    data, fmt, degree = small_v1("v1_hostile", 257)
    s = completed_stream(data, fmt, degree)
    with np.errstate(all="ignore"):
        f = s.fill(1, False, want_scale_rotation=True)
    s.close()
    assert np.isnan(f["centers"]).any() and np.isinf(f["centers"]).any()
    assert np.isinf(f["scales"]).any() and (f["scales"] == 0).any()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", ["v1_sh2", "ksplat"])
def test_a_range_beyond_the_ready_prefix_is_refused_and_changes_nothing(ctx, kind):
    data, fmt, degree = big_file(kind)
    stream = assets.SplatAssetStream(fmt, degree, len(data))
    stream.append(data[:len(data) // 2 + 13])
    ready = stream.stream_info.splats_ready
    assert 256 < ready < N
    pair = U.Pair(ctx, stream, ready + 16, False, True, False, 1)      # (16 slots more, so that the mesh's own bound is not what refuses)
    try:
        pair.device(0, 0, ready)
        pair.device(ready, 0, 16)
        before = pair.observe()
        assert before["frame"].any()
        for call in (lambda: stream.upload_to(pair.mesh, 0, ready - 5, 6), lambda: stream.upload_to(pair.mesh, 0, 0, ready + 1),
                     lambda: stream.upload_centers_to(pair.worker, 0, ready - 5, 6), lambda: stream.upload_centers_to(pair.worker, 0, ready, 1)):
            with pytest.raises(L.GsError, match="ready splats") as e:
                call()
            assert e.value.status == L.GS_ERR_INVALID
        assert stream.stream_info.splats_ready == ready
        U.assert_same(before, pair.observe(), "after the refused calls")
    finally:
        pair.close()
        stream.close()


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", ["v1_sh2", "v1_odd_stride"])
def test_encoding_a_completed_inria_v1_stream(ctx, name, level):
    """gs_asset_encode_ksplat reads the stream's rows through the INRIA-v1 source: byte for byte the encoding of the whole-file asset."""
    data, fmt, degree = small_v1(name, 257)
    whole, stream = assets.SplatAsset(data, fmt, degree), completed_stream(data, fmt, degree)
    try:
        ea, order_a = whole.encode_ksplat(ctx, level, 1, 2.0, 64)
        eb, order_b = stream.encode_ksplat(ctx, level, 1, 2.0, 64)
        assert np.array_equal(order_a, order_b)
        assert ea.to_bytes() == eb.to_bytes() and len(eb.to_bytes()) > 4096 + 1024
        ea.close()
        eb.close()
    finally:
        whole.close()
        stream.close()
