"""Streamed assets on the host (gs_asset_open_stream / gs_asset_append / gs_asset_get_stream_info; csrc/asset_stream.cpp and the
readers of csrc/assets.hip).  Rule M: once the final append is accepted the stream is the asset gs_asset_open returns for the
concatenated bytes.  Rule P: the ready splats are a prefix that never shrinks, and its length after every append is what a Python
model computes from the file's layout and the byte count (asset_stream_cases.Model - never from the library).  The GPU half is
tests/test_gpu_asset_stream.py."""
import ctypes as C
import struct

import numpy as np
import pytest

import asset_stream_cases as SC
from gaussiansplats3d_amd import GsError, assets
from gaussiansplats3d_amd import _lib as L
import test_assets_spz_open as SPZ
from test_assets_formats_open import edit_header

FILES = SC.files()
ARRAYS = ("centers", "cov", "cov_f16", "rgba", "sh_f16", "sh_u8", "scales", "rotations")
SMALLEST = 12_000                                # bytes: the files that are also fed byte by byte


def same_bits(a, b):
    """np.array_equal on the bytes: hostile files hold NaNs, which compare unequal to themselves."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def info_tuple(info):
    return (info.splat_count, info.sh_degree, info.compression_level, info.sh_level, tuple(info.scene_center), info.sh_min, info.sh_max)


def fills(asset, scale_rotation=True):
    with np.errstate(all="ignore"):
        out = [asset.fill(1, False, scale_rotation), asset.fill(40, True, False)]
    return out


def assert_same_asset(stream, whole, tag):
    assert info_tuple(stream.info) == info_tuple(whole.info), tag
    for a, b in zip(fills(stream), fills(whole)):
        for k in ARRAYS:
            assert same_bits(a[k], b[k]), f"{tag}: {k} differs between the stream and the whole-file asset"
    m = np.eye(4)
    ang = 0.3
    m[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ np.diag([1.2, 0.8, 1.1])
    m[:3, 3] = [0.5, -0.25, 2.0]
    stream.set_transform(m.T)
    whole.set_transform(m.T)
    assert info_tuple(stream.info) == info_tuple(whole.info), tag
    for a, b in zip(fills(stream, False), fills(whole, False)):
        for k in ARRAYS:
            assert same_bits(a[k], b[k]), f"{tag}: transformed {k} differs between the stream and the whole-file asset"
    stream.set_transform(None)
    whole.set_transform(None)


def open_stream(name):
    data, fmt, degree = FILES[name]
    return assets.SplatAssetStream(fmt, degree, len(data) if fmt == "splat" else 0)


def plans(name):
    data, fmt, degree = FILES[name]
    total, model = len(data), SC.Model(data, fmt, degree)
    out = {"whole": [total], "7": SC.by_size(total, 7), "4093": SC.by_size(total, 4093), "262144": SC.by_size(total, 262144),
           "borders": SC.around(total, model.borders)}
    if total <= SMALLEST:
        out["1"] = SC.by_size(total, 1)
    return out


CASES = [(name, plan) for name in sorted(FILES) for plan in plans(name)]


@pytest.fixture(scope="module")
def whole_assets():
    opened = {}

    def get(name):
        if name not in opened:
            data, fmt, degree = FILES[name]
            opened[name] = assets.SplatAsset(data, fmt, degree)
        return opened[name]
    yield get
    for a in opened.values():
        a.close()


@pytest.mark.parametrize("name,plan", CASES)
def test_ready_prefix_follows_the_model_and_the_end_is_the_whole_file(whole_assets, name, plan):
    """P after every append (against the model), M after the last (info and every fill array, again with a transform)."""
    data, fmt, degree = FILES[name]
    model, whole = SC.Model(data, fmt, degree), whole_assets(name)
    stream = open_stream(name)
    before = 0
    for received, final, info in SC.feed(stream, data, plans(name)[plan]):
        header, ready = model.at(received, final)
        if final:
            ready = whole.info.splat_count
        assert (info.bytes_received, bool(info.header_ready), info.splats_ready, bool(info.complete), info.failed) == \
            (received, header, ready, final, 0), f"{name}: after {received} bytes"
        assert info.splats_ready >= before
        before = info.splats_ready
        assert (stream.info is not None) == header
    assert_same_asset(stream, whole, name)
    stream.close()


def test_the_seeded_files_have_the_strides_and_the_early_rows_the_cases_need():
    """Some splats are ready before the end for the four formats that stream, none for .spz and INRIA-v2; the seeded INRIA-v1 files
    have the strides the kernel has to cope with."""
    for name, early in (("v1_sh2", True), ("pc_0_at_2", True), ("pc_24_at_0", True), ("splat_300", True), ("ksplat_l1_3sec", True),
                        ("spz_300", False), ("iv2_300", False)):
        data, fmt, degree = FILES[name]
        model = SC.Model(data, fmt, degree)
        assert (model.at(len(data) - 1)[1] > 0) == early, name
    strides = {name: SC.Model(*FILES[name]).runs[0][2] for name in SC.V1_CASES}
    assert strides["v1_sh0"] == 68 and strides["v1_sh3"] == 248 and strides["v1_odd_stride"] % 2 == 1 and strides["v1_rgb_no_scale"] == 31


# ------------------------------------------------------------------------------------------------ refusals
def last_error():
    return L.load().gs_last_error().decode()


def open_message(data, fmt, degree=2):
    """gs_asset_open's message for a file it refuses."""
    with pytest.raises(GsError) as e:
        assets.SplatAsset(data, fmt, degree)
    return str(e.value)


def append_refused(stream, data, final, message=None):
    before = stream.stream_info
    with pytest.raises(GsError) as e:
        stream.append(data, final)
    assert e.value.status == L.GS_ERR_INVALID
    if message is not None:
        assert str(e.value) == message
    after = stream.stream_info
    assert (after.bytes_received, after.header_ready, after.splats_ready, after.complete, after.failed) == \
        (before.bytes_received, before.header_ready, before.splats_ready, 0, 1), "a refused append consumes nothing and sets failed"
    with pytest.raises(GsError, match="refused an earlier append"):
        stream.append(b"", False)
    return str(e.value)


def test_a_rotation_nan_is_canonical_in_a_stream_and_everything_else_is_the_whole_files():
    """The one difference from gs_asset_open beside the exp: a NaN the quaternion normalisation makes (an infinite rot_*: inf * (1 / inf))
    or passes on (a NaN rot_*) is stored as the canonical quiet NaN by a streamed INRIA-v1 file, as every row source stores it,
    where parse_ply keeps the host's sign and payload.  Such rows are NaN in both, in the same places; every other value of every
    array is bit-equal."""
    data, fmt, degree = SC.v1_case("v1_nan_rotations")
    whole, stream = assets.SplatAsset(data, fmt, degree), open_stream_of(data, fmt, degree)
    for _ in SC.feed(stream, data, SC.by_size(len(data), 4093)):
        pass
    rows = np.array(SC.NAN_ROTATION_ROWS)
    row_s, row_w = (np.frombuffer(debug_row(a, int(rows[0])), np.uint32) for a in (stream, whole))
    assert (row_s[6:10] == 0x7FC00000).all(), "the stream's level-0 row holds the canonical NaN"
    assert np.isnan(row_w[6:10].view(np.float32)).all() and not (row_w[6:10] == 0x7FC00000).all(), "the case no longer tells the two apart"
    for a, b in zip(fills(stream), fills(whole)):
        for k in ARRAYS:
            if a[k] is None or b[k] is None:
                assert a[k] is None and b[k] is None
                continue
            nan = (lambda v: np.isnan(v.view(np.float16)) if v.dtype == np.uint16 else np.isnan(v)) if k not in ("rgba", "sh_u8") else (lambda v: np.zeros(v.shape, bool))
            na, nb = nan(a[k]), nan(b[k])
            assert np.array_equal(na, nb), f"{k}: NaN in different places"
            if k in ("cov", "cov_f16", "rotations"):
                assert na[rows].all() and not np.delete(na, rows, axis=0).any(), f"{k}: NaN exactly in the rows with a NaN / infinite rot_*"
            raw = (lambda v: v.view(np.uint32) if v.dtype == np.float32 else v)
            assert np.array_equal(raw(a[k])[~na], raw(b[k])[~nb]), f"{k} differs outside the NaNs"
    whole.close()
    stream.close()


def open_stream_of(data, fmt, degree):
    return assets.SplatAssetStream(fmt, degree, len(data) if fmt == "splat" else 0)


def test_splat_needs_expected_bytes_and_takes_no_more():
    with pytest.raises(GsError, match="expected_bytes"):
        assets.SplatAssetStream("splat", 0, 0)
    assert open_message(bytes(33), "splat") in _raises(lambda: assets.SplatAssetStream("splat", 0, 33))
    data = FILES["splat_300"][0]
    s = assets.SplatAssetStream("splat", 0, len(data))
    assert s.info.splat_count == 300 and s.stream_info.header_ready == 1
    s.append(data[:100])
    assert s.stream_info.splats_ready == 3
    append_refused(s, data[100:] + b"\0", False)
    assert s.stream_info.splats_ready == 3
    s.close()


def _raises(f):
    with pytest.raises(GsError) as e:
        f()
    return str(e.value)


def test_unknown_format():
    lib, handle = L.load(), C.c_void_p(0xDEAD)
    assert lib.gs_asset_open_stream(9, 2, 0, C.byref(handle)) == L.GS_ERR_INVALID and handle.value is None
    assert "unknown asset format" in last_error()
    with pytest.raises(ValueError):
        assets.SplatAssetStream("obj")


def debug_row(asset, splat):
    """gs_debug_asset_row: splat `splat` of the ready prefix as the host decodes it out of the bytes that have arrived, or None."""
    fn = L.load().gs_debug_asset_row
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    out, size = C.create_string_buffer(256), C.c_uint32()
    return out.raw[:size.value] if fn(asset.handle, splat, out, C.byref(size)) == L.GS_OK else None


SHORT = ["v1_sh1", "v1_odd_stride", "pc_9_at_2", "pc_0_at_2", "splat_300", "ksplat_l0_3sec", "ksplat_l2_3sec", "spz_300", "iv2_300",
         "iv2_300_codebook_first"]


@pytest.mark.parametrize("name", SHORT)
def test_final_on_a_short_file(name):
    """Every format: the file ends one byte early (and, for a second stream, in the middle).  The final append is refused - with
    gs_asset_open's message for the short file where it has one - and the ready rows stay what they were."""
    data, fmt, degree = FILES[name]
    model = SC.Model(data, fmt, degree)
    for cut in (len(data) - 1, len(data) * 2 // 3):
        s = open_stream(name)
        s.append(data[:cut // 2])
        # (a short .splat is a shorter .splat to gs_asset_open; the stream knows the count from expected_bytes)
        expect = None if fmt == "splat" else open_message(data[:cut], fmt, degree)
        message = append_refused(s, data[cut // 2:cut], True, expect)
        assert message
        info = s.stream_info
        assert info.splats_ready == model.at(cut // 2)[1] and info.complete == 0
        whole = assets.SplatAsset(data, fmt, degree)         # the ready rows still decode, to what the whole file gives for them
        for i in sorted({0, 1, info.splats_ready // 2, info.splats_ready - 1} & set(range(info.splats_ready))):
            assert debug_row(s, i) == debug_row(whole, i), (name, i)
        assert debug_row(s, info.splats_ready) is None
        whole.close()
        assert L.load().gs_asset_fill(s.handle, 1, *[None] * 8) == L.GS_ERR_INVALID and "not complete" in last_error()
        s.close()


def _v1(n_rest=9):
    return SC.v1_file(64, n_rest, 5)


def _patch(data, at, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def _pc():
    return FILES["pc_9_at_2"][0]


def _ks():
    return FILES["ksplat_l1_3sec"][0]


def _v2():
    return FILES["iv2_300"][0]


def _spz_payload():
    return SPZ.stream(300, 1)


def _ks_full_buckets_overflow():
    """Section 0 claims 65 000 full buckets of 70 000 splats among 70 000 stored ones; the file is padded so that they fit."""
    d = _patch(_patch(_patch(_ks(), 4096 + 8, "<I", 70_000), 4096 + 12, "<I", 70_000), 4096 + 32, "<I", 65_000)
    return d + bytes(1 << 20)


def _ks_partial_overflow():
    assert struct.unpack_from("<I", _ks(), 4096 + 36)[0] >= 1 and struct.unpack_from("<I", _ks(), 4096 + 32)[0] >= 1
    return _patch(_ks(), 4096 + 3 * 1024, "<I", 0xFFFFFFFF)              # the first partial bucket's length


def _pc_wide_chunk_row():
    wide = "".join(f"property double w{k}\n" for k in range(1 << 21))     # 16 MiB of doubles in a chunk row
    return edit_header(_pc(), "element vertex 600", wide + "element vertex 600")


V2_PAD = bytes(1 << 16)                  # behind the last element: a header edit that widens a row still finds its data
WIDE = "".join(f"property double w{k}\n" for k in range(8192))

# Every fault gs_asset_open names, per format: name -> (the file, fmt, words of the message, when the stream must refuse it).
# "header": with the append that completes the header (or the section's tables) - before the final one when the file comes in
# pieces; "final": only the final append can know (the file's end, a gzip member's trailer, a codebook behind the rows);
# None: a header as long as the file, nothing to tell apart.
HEADER_FAULTS = {
    "v1_unsized_property": (lambda: edit_header(_v1(), "property float nx", "property list nx"), "ply", "PLY: property type", "header"),
    "v1_no_end_header": (lambda: _v1()[:200] + bytes(1 << 20) + bytes(5000), "ply", "PLY: end_header not found", "header"),
    "v1_vertex_data": (lambda: _v1()[:-1], "ply", "PLY: vertex data exceeds the file", "final"),
    "pc_no_ply_magic": (lambda: b"plx\n" + _pc()[4:], "ply", "does not start with 'ply'", "header"),
    "pc_no_end_of_header": (lambda: _pc().replace(b"end_header\n", b"end_header \n", 1), "ply", "compressed PLY: end of header not found", "final"),
    "pc_format_ascii": (lambda: edit_header(_pc(), "format binary_little_endian 1.0", "format ascii 1.0"), "ply", "not binary_little_endian", "header"),
    "pc_element_count": (lambda: edit_header(_pc(), "element sh 600", "element sh x"), "ply", "compressed PLY: an element count", "header"),
    "pc_property_type": (lambda: edit_header(_pc(), "property uchar f_rest_3", "property uint8 f_rest_3"), "ply", "unrecognized property data type", "header"),
    "pc_property_before_element": (lambda: edit_header(_pc(), "element chunk 3\n", "property float q\nelement chunk 3\n"), "ply",
                                   "compressed PLY: a property precedes every element", "header"),
    "pc_obj_info": (lambda: edit_header(_pc(), "element chunk", "obj_info made elsewhere\nelement chunk"), "ply", "unrecognized header value", "header"),
    "pc_elements_order": (lambda: edit_header(_pc(), "element chunk 3", "element chunks 3"), "ply", "must begin with chunk, vertex", "header"),
    "pc_repeated_element": (lambda: edit_header(_pc(), "property uchar f_rest_8\n", "property uchar f_rest_8\nelement vertex 0\n"), "ply",
                            "repeated or out of order", "header"),
    "pc_wide_row": (_pc_wide_chunk_row, "ply", "an element row of 16 MiB or more", None),
    "pc_element_data": (lambda: _pc()[:-1], "ply", "compressed PLY: element data exceeds the file", "final"),
    "pc_fewer_chunks": (lambda: edit_header(_pc(), "element chunk 3", "element chunk 2"), "ply", "fewer chunks", "header"),
    "pc_vertex_row": (lambda: edit_header(_pc(), "property uint packed_scale\n", ""), "ply", "not the four packed uints", "header"),
    "pc_packed_type": (lambda: edit_header(_pc(), "property uint packed_color", "property float packed_color"), "ply", "missing or not uint", "header"),
    "pc_extreme_type": (lambda: edit_header(_pc(), "property float max_x", "property int max_x"), "ply", "a chunk extreme is not float", "header"),
    "pc_extreme_missing": (lambda: edit_header(_pc(), "property float min_scale_y", "property float min_scale_q"), "ply", "extreme is missing", "header"),
    "pc_sh_count": (lambda: edit_header(_pc(), "element sh 600", "element sh 599"), "ply", "count differs from the vertex count", "header"),
    "pc_sh_names": (lambda: edit_header(_pc(), "property uchar f_rest_3", "property uchar f_rest_x"), "ply", "is not f_rest_0 .. f_rest_N-1", "header"),
    "ksplat_short_header": (lambda: _ks()[:4000], "ksplat", "shorter than its 4096-byte header", "final"),
    "ksplat_section_headers": (lambda: _ks()[:4096 + 2 * 1024 + 10], "ksplat", "section headers exceed the file", "final"),
    "ksplat_section_data": (lambda: _ks()[:-1], "ksplat", "section data exceeds the file", "final"),
    "ksplat_level": (lambda: _patch(_ks(), 20, "<H", 3), "ksplat", "unknown compression level", "header"),
    "ksplat_sh_degree": (lambda: _patch(_ks(), 4096 + 2 * 1024 + 40, "<H", 3), "ksplat", "spherical harmonics degree > 2", "header"),
    "ksplat_counts_disagree": (lambda: _patch(_ks(), 12, "<I", 700), "ksplat", "splat counts disagree", "header"),
    "ksplat_bucket_storage": (lambda: _patch(_ks(), 4096 + 20, "<H", 8), "ksplat", "bucket storage below", "header"),
    "ksplat_bucket_size": (lambda: _patch(_ks(), 4096 + 8, "<I", 0), "ksplat", "bucket size 0", "header"),
    "ksplat_full_plus_partial": (lambda: _patch(_ks(), 4096 + 32, "<I", 1000), "ksplat", "more full + partial buckets", "header"),
    "ksplat_full_overflow": (_ks_full_buckets_overflow, "ksplat", "full buckets x bucket size overflows 32 bits", "header"),
    "ksplat_partial_overflow": (_ks_partial_overflow, "ksplat", "partial bucket lengths overflow", "header"),
    "ksplat_buckets_cover": (lambda: _patch(_ks(), 4096 + 32, "<I", 0), "ksplat", "do not cover every splat", "header"),
    # INRIA-v2: the whole-file parser runs at the final append (the codebook may lie behind the rows)
    "v2_no_end_header": (lambda: _v2()[:_v2().index(b"end_header")] + bytes(4096), "ply", "INRIA-v2 PLY: end_header not found", "final"),
    "v2_format": (lambda: edit_header(_v2(), "format binary_little_endian 1.0", "format ascii 1.0"), "ply", "INRIA-v2 PLY: the format", "final"),
    "v2_element_count": (lambda: edit_header(_v2(), "element vertex 300", "element vertex many"), "ply", "INRIA-v2 PLY: an element count", "final"),
    "v2_unsized_property": (lambda: edit_header(_v2(), "element codebook_centers", "property char pad\nelement codebook_centers") + V2_PAD, "ply",
                            "INRIA-v2 PLY: property type", "final"),
    "v2_property_before_element": (lambda: edit_header(_v2(), "format binary_little_endian 1.0\n", "format binary_little_endian 1.0\nproperty short q\n"),
                                   "ply", "INRIA-v2 PLY: a property precedes every element", "final"),
    "v2_wide_row": (lambda: edit_header(_v2(), "element codebook_centers", WIDE + "element codebook_centers"), "ply", "INRIA-v2 PLY: an element row of 64 KiB", "final"),
    "v2_element_data": (lambda: _v2()[:-1], "ply", "INRIA-v2 PLY: element data exceeds the file", "final"),
    "v2_third_element": (lambda: edit_header(_v2(), "property short rotation_im\n", "property short rotation_im\nelement face 0\n"), "ply",
                         "more than one", "final"),
    "v2_no_codebook": (lambda: b"ply\nformat binary_little_endian 1.0\nelement codebook_centers_x 256\nproperty short scaling\nend_header\n" + bytes(512),
                       "ply", "no codebook_centers element", "final"),
    "v2_no_vertex": (lambda: b"ply\nformat binary_little_endian 1.0\nelement codebook_centers 256\nproperty short scaling\nend_header\n" + bytes(512),
                     "ply", "no element besides codebook_centers", "final"),
    "v2_codebook_rows": (lambda: edit_header(_v2(), "element codebook_centers 256", "element codebook_centers 255"), "ply", "fewer than 256", "final"),
    "v2_centre_type": (lambda: edit_header(_v2(), "property short y", "property float y") + V2_PAD, "ply", "x / y / z are not short / ushort", "final"),
    "v2_index_type": (lambda: edit_header(_v2(), "property uchar f_rest_4\n", "property ushort f_rest_4\n") + V2_PAD, "ply", "is not uchar", "final"),
    "v2_f_rest_count": (lambda: edit_header(_v2(), "property uchar f_rest_8\n", "property uchar other_8\n"), "ply", "the f_rest_* fields are not", "final"),
    "v2_centre_missing": (lambda: edit_header(_v2(), "property short z\n", "property short zq\n"), "ply", "x / y / z missing", "final"),
    "v2_rotation_missing": (lambda: edit_header(_v2(), "property uchar rot_2\n", "property uchar rot_2q\n"), "ply", "rot_0 .. rot_3 missing", "final"),
    "v2_page_missing": (lambda: edit_header(_v2(), "property short scaling\n", "property short scaling_\n"), "ply", "a codebook page that", "final"),
    "v2_page_type": (lambda: edit_header(_v2(), "property short opacity\n", "property float opacity\n") + V2_PAD, "ply", "a codebook property is not short", "final"),
    # .spz: a gzip member ends in its CRC - every refusal of the container comes with the final append
    "spz_short_gzip_header": (lambda: b"\x1f\x8b\x08", "spz", "shorter than a gzip header", "final"),
    "spz_not_gzip": (_spz_payload, "spz", "does not start with 1f 8b", "final"),
    "spz_method": (lambda: SPZ.member(_spz_payload())[:2] + b"\x07" + SPZ.member(_spz_payload())[3:], "spz", "not deflate", "final"),
    "spz_reserved_flag": (lambda: SPZ.member(_spz_payload())[:3] + b"\x20" + SPZ.member(_spz_payload())[4:], "spz", "reserved gzip flag", "final"),
    "spz_gzip_header_short": (lambda: SPZ.member(_spz_payload(), flags=4, extra=b"xy")[:11], "spz", "the gzip header ends short", "final"),
    "spz_header_crc16": (lambda: SPZ.member(_spz_payload(), flags=2)[:10] + b"\0\0" + SPZ.member(_spz_payload(), flags=2)[12:], "spz", "CRC-16", "final"),
    "spz_stored_complement": (lambda: _patch(SPZ.member(_spz_payload(), level=0), 13, "<H", 0), "spz", "length and its complement disagree", "final"),
    "spz_block_type_3": (lambda: SPZ.member(_spz_payload())[:10] + b"\x07" + bytes(20), "spz", "reserved type 3", "final"),
    "spz_deflate_short": (lambda: SPZ.member(_spz_payload())[:-200], "spz", ".spz:", "final"),
    "spz_magic": (lambda: SPZ.member(SPZ.with_header(_spz_payload(), magic=1347635021)), "spz", "wrong magic", "final"),
    "spz_version": (lambda: SPZ.member(SPZ.with_header(_spz_payload(), version=3)), "spz", "version not supported", "final"),
    "spz_points": (lambda: SPZ.member(SPZ.with_header(_spz_payload(), n=10_000_001)), "spz", "too many points", "final"),
    "spz_sh_degree": (lambda: SPZ.member(SPZ.with_header(_spz_payload(), degree=4)), "spz", "unsupported SH degree", "final"),
    "spz_no_spz_header": (lambda: SPZ.member(_spz_payload()[:15]), "spz", "shorter than the 16-byte SPZ header", "final"),
    "spz_planes_short": (lambda: SPZ.member(_spz_payload()[:-1]), "spz", "incorrect size", "final"),
    "spz_planes_long": (lambda: SPZ.member(_spz_payload() + b"\0"), "spz", "more bytes than the header implies", "final"),
    "spz_trailer_short": (lambda: SPZ.member(_spz_payload())[:-3], "spz", "the gzip trailer is cut short", "final"),
    "spz_crc32": (lambda: SPZ.member(_spz_payload(), crc=1), "spz", "wrong CRC-32", "final"),
    "spz_isize": (lambda: SPZ.member(_spz_payload(), isize=7), "spz", "wrong ISIZE", "final"),
    "spz_trailing_bytes": (lambda: SPZ.member(_spz_payload()) + b"\0", "spz", "trailing bytes", "final"),
}
FAULT_SIZES = {"pc_wide_row": [1 << 30, 1 << 22]}            # (a 36 MB header: whole and in 4 MiB appends)


def c_open_message(data, fmt):
    """gs_asset_open's refusal of `data`, asked of the library itself (SplatAsset looks at an .spz's magic before it calls)."""
    lib, handle = L.load(), C.c_void_p()
    buf = (C.c_char * max(len(data), 1)).from_buffer_copy(data or b"\0")
    assert lib.gs_asset_open(buf, len(data), assets.SplatAsset.FORMATS[fmt], 2, C.byref(handle)) == L.GS_ERR_INVALID
    return f"libgsplat_hip status -1: {last_error()}"


@pytest.mark.parametrize("fault", sorted(HEADER_FAULTS))
@pytest.mark.parametrize("size", [1 << 30, 4093, 97])
def test_a_damaged_file_is_refused_with_the_message_of_gs_asset_open(fault, size):
    """The append that makes the refusal certain carries gs_asset_open's message - whole, in 4093-byte and in 97-byte appends.  A
    header fault comes with the header, before the file has ended; what only the end of the file can show comes with the final
    append and not before.  Nothing is consumed, nothing is ready that the whole-file reader would not have given."""
    make, fmt, words, when = HEADER_FAULTS[fault]
    if size not in FAULT_SIZES.get(fault, [size]):
        size = FAULT_SIZES[fault][-1]
    data = make()
    expect = c_open_message(data, fmt)
    assert words in expect, (fault, expect)
    s = assets.SplatAssetStream(fmt, 2)
    ends = SC.by_size(len(data), min(size, len(data)))
    at = 0
    for k, end in enumerate(ends):
        final = k == len(ends) - 1
        try:
            s.append(data[at:end], final)
        except GsError as e:
            assert str(e) == expect, fault
            info = s.stream_info
            assert info.failed == 1 and info.complete == 0 and info.bytes_received == at
            if when == "final":
                assert final, f"{fault}: refused after {end} of {len(data)} bytes, before the file had ended"
            if when == "header" and len(ends) > 2:
                assert not final, f"{fault}: a header fault was only refused with the final append"
            break
        at = end
    else:
        raise AssertionError(f"{fault}: every append was accepted")
    if when == "header" and not fault.startswith("ksplat_"):     # (a .ksplat's earlier sections and a short file's rows are ready, and stay)
        assert s.stream_info.splats_ready == 0
    s.close()


def test_every_message_of_the_readers_has_a_case():
    """The table above against the source: every refusal the six readers of csrc/assets.hip and the container checks of
    csrc/spz_container.hpp can name is asked for by a case - apart from the deflate decoder's own (a damaged code table is the
    inflate's business at the final append, like the CRC that follows it), the 2^32-row .splat (no such file fits) and the .splat
    length (a stream is refused at open: test_splat_needs_expected_bytes_and_takes_no_more)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussiansplats3d_amd", "csrc")
    text = open(os.path.join(csrc, "assets.hip")).read()
    named = set(re.findall(r'"((?:\.ksplat|compressed PLY|INRIA-v2 PLY|PLY): [^"]*)"', text))
    named |= {m for m in re.findall(r'return "(\.spz: [^"]*)"', open(os.path.join(csrc, "spz_container.hpp")).read())
              if not re.search(r"block|symbol|deflate stream|before the start", m)}
    named -= {"PLY: a vertex row of 64 KiB or more"}        # the stream's own: test_a_row_of_64_kib_is_refused_by_the_stream
    assert len(named) > 60
    messages = [c_open_message(make(), fmt) for name, (make, fmt, _, _) in HEADER_FAULTS.items() if name != "pc_wide_row"]
    messages.append("compressed PLY: an element row of 16 MiB or more")      # (its 36 MB file is opened once, by the test above)
    missing = sorted(m for m in named if not any(m in got for got in messages))
    assert not missing, missing


def test_header_faults_surface_with_the_header():
    """A header fault is refused by the append that completes the header, not at the end of the file."""
    data, fmt = HEADER_FAULTS["pc_extreme_type"][0](), "ply"
    end = data.index(b"end_header\n") + 11
    s = assets.SplatAssetStream(fmt, 2)
    s.append(data[:end - 1])
    assert s.stream_info.header_ready == 0 and s.info is None
    append_refused(s, data[end - 1:end + 5], False, open_message(data, fmt))
    s.close()
    data, fmt = HEADER_FAULTS["ksplat_sh_degree"][0](), "ksplat"
    s = assets.SplatAssetStream(fmt, 2)
    s.append(data[:4096 + 3 * 1024 - 1])
    append_refused(s, data[4096 + 3 * 1024 - 1:4096 + 3 * 1024], False, open_message(data, fmt))
    s.close()


def test_a_bucket_table_fault_keeps_the_sections_before_it():
    """The tables of the third section are damaged: the first section's rows were ready before and stay ready."""
    data = FILES["ksplat_l1_3sec"][0]
    bad = _patch(data, 4096 + 2 * 1024 + 32, "<I", 1000)                        # section 2: more full buckets than it stores
    model = SC.Model(data, "ksplat", 2)
    s = assets.SplatAssetStream("ksplat", 2)
    first_rows_end = model.runs[0][1] + model.runs[0][2] * model.runs[0][3]
    s.append(bad[:first_rows_end])
    assert s.stream_info.splats_ready == 301
    append_refused(s, bad[first_rows_end:], False, open_message(bad, "ksplat"))
    assert s.stream_info.splats_ready == 301
    s.close()


def test_no_end_header_within_the_first_mib():
    s = assets.SplatAssetStream("ply", 2)
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 1\n"
    s.append(head + b"comment " + b"x" * ((1 << 20) - len(head) - 9))
    assert s.stream_info.failed == 0 and s.stream_info.header_ready == 0
    append_refused(s, b"x", False, "libgsplat_hip status -1: invalid argument: PLY: end_header not found")
    s.close()


def test_append_after_complete_and_empty_appends():
    data, fmt, degree = FILES["v1_sh1"]
    s = assets.SplatAssetStream(fmt, degree, len(data))
    s.append(b"")
    s.append(data[:1000])
    s.append(b"")
    assert s.stream_info.bytes_received == 1000
    s.append(data[1000:])
    assert s.stream_info.complete == 0 and s.stream_info.splats_ready == 257
    with pytest.raises(GsError, match="not complete"):
        s.fill()
    s.append(b"", True)
    assert s.stream_info.complete == 1
    with pytest.raises(GsError, match="complete"):
        s.append(b"", False)
    info = s.stream_info
    assert (info.complete, info.failed, info.splats_ready) == (1, 1, 257)
    s.fill()                                                 # the completed asset is still the asset
    s.close()


def test_fill_and_get_info_before_their_time():
    data, fmt, degree = FILES["ksplat_l1_3sec"]
    lib = L.load()
    s = assets.SplatAssetStream(fmt, degree)
    info = L.AssetInfo()
    assert lib.gs_asset_get_info(s.handle, C.byref(info)) == L.GS_ERR_INVALID and "header" in last_error()
    s.append(data[:5000])
    assert s.info is None
    s.append(data[5000:-1])
    assert s.info.splat_count == 611
    with pytest.raises(GsError, match="not complete"):
        s.fill()
    handle = C.c_void_p()
    p = L.KsplatParams(1, 1, 256, 5.0, (C.c_float * 3)(0, 0, 0), 0)
    assert lib.gs_asset_encode_ksplat(None, s.handle, C.byref(p), C.byref(handle), None) == L.GS_ERR_INVALID   # (a level-1 file: asked before the level)
    assert "not complete" in last_error()
    s.close()
    data, fmt, degree = FILES["v1_sh0"]
    s = assets.SplatAssetStream(fmt, degree)
    s.append(data[:-1])
    assert lib.gs_asset_encode_ksplat(None, s.handle, C.byref(p), C.byref(handle), None) == L.GS_ERR_INVALID
    assert "not complete" in last_error()
    s.close()


def test_stream_calls_on_an_opened_asset():
    data, fmt, degree = FILES["v1_sh0"]
    a = assets.SplatAsset(data, fmt, degree)
    lib = L.load()
    assert lib.gs_asset_append(a.handle, b"x", 1, 0) == L.GS_ERR_INVALID and "no stream" in last_error()
    assert lib.gs_asset_get_stream_info(a.handle, C.byref(L.AssetStreamInfo())) == L.GS_ERR_INVALID
    a.close()


def test_a_row_of_64_kib_is_refused_by_the_stream():
    props = "".join(f"property double pad{k}\n" for k in range(8192))
    data = ("ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\n" + props + "end_header\n").encode()
    s = assets.SplatAssetStream("ply", 2)
    assert "64 KiB" in append_refused(s, data, False)
    s.close()


def test_the_symbols_are_in_the_header_and_the_table():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gsplat_hip.h")).read()
    for name in ("gs_asset_open_stream", "gs_asset_append", "gs_asset_get_stream_info"):
        assert f"int {name}(" in text and name in L.SYMBOLS
    assert L.load().gs_abi_version() == 5
