"""gs_asset_open on INRIA-v2 codebook PLY files (parse_inria_v2 of csrc/assets.hip): every refusal (GS_ERR_INVALID, a message that
begins `INRIA-v2 PLY:`, `out` left NULL - everything the row decode relies on is proven at open), what opens all the same, the
writer of gaussiansplats3d_amd.assets through the reader, and a damage run of seeded mutations of a valid file."""
import numpy as np
import pytest

from gaussiansplats3d_amd import _lib as L
from gaussiansplats3d_amd import assets
from test_assets_formats_open import edit_header, open_status

SH_C0 = 0.28209479177387814
N = 600


def inputs(n=N, ncoef=9, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)), rng.normal(-3.0, 0.5, size=(n, 3)), rng.normal(size=(n, 4)), rng.normal(0.0, 1.0, size=(n, 3)),
            rng.normal(0.0, 2.0, size=n), rng.normal(0.0, 0.5, size=(n, ncoef)) if ncoef else None)


_FILES = {}


def v2(ncoef=9, **kw):
    key = repr((ncoef, sorted(kw.items())))
    if key not in _FILES:
        _FILES[key] = assets.write_inria_v2_ply(*inputs(ncoef=ncoef), **kw)
    return _FILES[key]


def refused(data, fragment):
    """GS_ERR_INVALID, `out` NULL, and the message: the `INRIA-v2 PLY:` prefix (behind GS_ERR_INVALID's own words) and the reason."""
    st, handle = open_status(data, L.GS_ASSET_PLY)
    message = L.load().gs_last_error().decode()
    assert st == L.GS_ERR_INVALID and handle is None, (st, handle)
    assert message.startswith("invalid argument: INRIA-v2 PLY:") and fragment in message, message


def opens(data, degree=2):
    a = assets.SplatAsset(data, "ply", degree)
    try:
        with np.errstate(all="ignore"):
            return a.info.splat_count, a.info.sh_degree, a.fill(1, False, want_scale_rotation=True)
    finally:
        a.close()


PAD = bytes(1 << 16)                      # behind the last element: a header edit that widens a row still finds its data


# ------------------------------------------------------------------------------------------------ refusals
def test_format_ascii():
    refused(edit_header(v2(), "format binary_little_endian 1.0", "format ascii 1.0"), "binary_little_endian")
    refused(edit_header(v2(), "format binary_little_endian 1.0", "format binary_big_endian 1.0"), "binary_little_endian")


def test_no_end_header():
    data = v2()
    refused(data[:data.index(b"end_header")] + bytes(4096), "end_header")


@pytest.mark.parametrize("line", ["property char pad", "property list uchar int idx", "property uint8 pad"])
def test_an_unsized_property_type(line):
    refused(edit_header(v2(), "element codebook_centers", line + "\nelement codebook_centers") + PAD, "does not size")
    refused(edit_header(v2(), "property short rotation_im\n", "property short rotation_im\n" + line + "\n") + PAD, "does not size")


@pytest.mark.parametrize("count", ["many", "-1", "4294967296", "99999999999999999999"])
def test_an_element_count_that_is_no_number_below_2_32(count):
    refused(edit_header(v2(), "element vertex 600", f"element vertex {count}"), "element count")
    refused(edit_header(v2(), "element codebook_centers 256", f"element codebook_centers {count}"), "element count")


def test_more_than_one_element_besides_the_codebook_or_none():
    refused(edit_header(v2(), "property short rotation_im\n", "property short rotation_im\nelement face 0\n"), "more than one")
    refused(edit_header(v2(codebook_first=True), "element vertex 600", "element vertex 300\nproperty uchar pad\nelement more 1"), "more than one")
    refused(edit_header(v2(), "element vertex 600", "element codebook_centers 600"), "more than one")
    refused(b"ply\nformat binary_little_endian 1.0\nelement codebook_centers 256\nproperty short scaling\nend_header\n" + bytes(512),
            "no element besides")


@pytest.mark.parametrize("name", ["x", "y", "z", "rot_0", "rot_1", "rot_2", "rot_3"])
def test_a_centre_or_rotation_field_is_missing(name):
    typ = "short" if name in "xyz" else "uchar"
    refused(edit_header(v2(), f"property {typ} {name}\n", f"property {typ} {name}q\n"), "missing")


@pytest.mark.parametrize("typ", ["float", "uchar", "int", "double"])
def test_a_centre_field_that_is_no_half(typ):
    refused(edit_header(v2(), "property short y", f"property {typ} y") + PAD, "x / y / z are not short / ushort")


@pytest.mark.parametrize("name", ["f_dc_1", "f_rest_4", "opacity", "scale_2", "rot_0"])
def test_an_index_field_that_is_not_uchar(name):
    refused(edit_header(v2(), f"property uchar {name}\n", f"property ushort {name}\n") + PAD, "is not uchar")


@pytest.mark.parametrize("drop", [1, 2, 8])
def test_an_f_rest_count_outside_0_9_24_45(drop):
    data = v2()
    for k in range(drop):
        data = edit_header(data, f"property uchar f_rest_{8 - k}\n", f"property uchar other_{k}\n")
    refused(data, "f_rest")
    refused(edit_header(v2(), "property uchar opacity", "property uchar f_rest_9\nproperty uchar opacity") + PAD, "f_rest")


@pytest.mark.parametrize("page", ["features_dc", "features_rest_2", "opacity", "scaling", "rotation_re", "rotation_im"])
def test_a_codebook_page_that_is_no_half(page):
    refused(edit_header(v2(), f"property short {page}\n", f"property float {page}\n") + PAD, "codebook property is not short / ushort")


def test_fewer_than_256_codebook_rows():
    refused(edit_header(v2(), "element codebook_centers 256", "element codebook_centers 255"), "fewer than 256")
    refused(edit_header(v2(), "element codebook_centers 256", "element codebook_centers 0"), "fewer than 256")


@pytest.mark.parametrize("page,ncoef", [("features_dc", 0), ("opacity", 0), ("scaling", 0), ("rotation_re", 0), ("rotation_im", 0),
                                        ("features_rest_0", 9), ("features_rest_2", 9), ("features_rest_3", 24), ("features_rest_7", 45)])
def test_a_codebook_page_that_the_fields_need_is_missing(page, ncoef):
    refused(edit_header(v2(ncoef), f"property short {page}\n", f"property short {page}_\n"), "page")
    refused(assets.write_inria_v2_ply(*inputs(ncoef=ncoef), codebook_override={page: None}), "page")


def test_element_data_beyond_the_end_of_the_file():
    for data in (v2(), v2(codebook_first=True)):
        refused(data[:-1], "exceeds the file")
        refused(data[:data.index(b"end_header\n") + 11 + 100], "exceeds the file")
        refused(data[:data.index(b"end_header\n") + 10], "exceeds the file")
    refused(edit_header(v2(), "element vertex 600", "element vertex 601"), "exceeds the file")


def test_a_row_of_64_kib_or_more():
    wide = "".join(f"property double w{k}\n" for k in range(8192))
    refused(edit_header(v2(), "element codebook_centers", wide + "element codebook_centers"), "64 KiB")
    refused(edit_header(v2(), "property short rotation_im\n", "property short rotation_im\n" + wide), "64 KiB")
    small = assets.write_inria_v2_ply(*inputs(n=4))
    almost = "".join(f"property double w{k}\n" for k in range(8188))                   # 65 504 + 26 bytes: still a row
    assert opens(edit_header(small, "property short x\n", almost + "property short x\n") + bytes(8188 * 8 * 4))[0] == 4


# ------------------------------------------------------------------------------------------------ what opens
def test_both_element_orders_open_and_read_the_same():
    a, b = opens(v2()), opens(v2(codebook_first=True))
    assert a[:2] == b[:2] == (N, 1)
    for k in ("centers", "cov", "rgba", "sh_f16", "scales", "rotations"):
        assert np.array_equal(a[2][k], b[2][k]), k


def test_what_nothing_reads_may_be_anything():
    """Extra properties only move offsets, comments are dropped, pages and fields beyond the second band are not looked at, a file
    without scale / colour / opacity fields needs none of their pages."""
    plain = opens(v2())[2]
    order = [f"f_rest_{k}" for k in range(9)] + ["pad", "rot_3", "rot_2", "rot_1", "rot_0", "z", "y", "x", "scale_1", "scale_0", "scale_2",
                                                 "opacity", "f_dc_2", "f_dc_1", "f_dc_0", "more"]
    other = opens(v2(half_type="ushort", comment="element vertex 5", extra_vertex=[("double", "pad"), ("uchar", "more")],
                     extra_codebook=[("float", "spare"), ("uchar", "features_rest_15")], field_order=order))[2]
    for k in ("centers", "cov", "rgba", "sh_f16", "scales", "rotations"):
        assert np.array_equal(plain[k], other[k]), k
    data45 = assets.write_inria_v2_ply(*inputs(ncoef=45), codebook_override={f"features_rest_{k}": None for k in range(8, 15)})
    assert opens(data45)[:2] == (N, 2)
    c, ls, q, dc, op, _ = inputs(ncoef=0)
    bare = assets.write_inria_v2_ply(c, None, q, None, None, codebook_override={"features_dc": None, "opacity": None, "scaling": None})
    n, degree, f = opens(bare)
    assert (n, degree) == (N, 0) and (f["scales"] == np.float32(0.01)).all() and not f["rgba"].any()


def test_a_missing_sh_field_reads_as_zero():
    """f_rest_4 renamed (the count stays 9): the reference reads `undefined || 0` for level-0 slots 4 (channel 1, coefficient 1)."""
    whole = opens(v2())[2]["sh_f16"]
    holed = opens(edit_header(v2(), "property uchar f_rest_4\n", "property uchar f_rest_x\n"))[2]["sh_f16"]
    slot = 3 * 1 + 1                                                                  # the fill's order: coefficient-major, RGB interleaved
    assert not holed[:, slot].any() and whole[:, slot].any()
    keep = np.arange(9) != slot
    assert np.array_equal(holed[:, keep], whole[:, keep])


def test_the_output_degree_is_the_smallest_of_requested_file_and_2():
    for ncoef, file_degree in ((0, 0), (9, 1), (24, 2), (45, 2)):
        for want in (0, 1, 2, 3):
            assert opens(v2(ncoef), want)[:2] == (N, min(want, file_degree))


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("ncoef,degree", [(0, 0), (9, 1), (24, 2), (45, 2)])
def test_write_inria_v2_ply_round_trips(ncoef, degree):
    """What opens is, value by value, the nearest codebook entry of what was written."""
    c, ls, q, dc, op, rest = inputs(ncoef=ncoef)
    n, deg, f = opens(v2(ncoef))
    assert (n, deg) == (N, degree)
    assert np.array_equal(f["centers"], c.astype(np.float16).astype(np.float32))

    def nearest(values):
        entries, index = assets._codebook_page(values)
        e = entries.astype(np.float64)
        v = np.asarray(values, np.float64)
        assert np.array_equal(np.abs(e[index] - v), np.abs(e[None, :] - v.reshape(-1, 1)).min(axis=1).reshape(v.shape))
        return e[index]

    assert np.allclose(f["scales"], np.exp(nearest(ls)), rtol=1e-6, atol=0)
    want_rgb = np.clip(np.floor(np.floor((0.5 + SH_C0 * nearest(dc)) * 255 + 0.5)), 0, 255)
    want_a = np.clip(np.floor(np.floor(1 / (1 + np.exp(-nearest(op))) * 255 + 0.5)), 0, 255)
    assert np.array_equal(f["rgba"][:, :3], want_rgb.astype(np.uint8)) and np.array_equal(f["rgba"][:, 3], want_a.astype(np.uint8))
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    coded = np.concatenate([nearest(qn[:, :1]), nearest(qn[:, 1:])], axis=1)
    coded = coded / np.linalg.norm(coded, axis=1, keepdims=True)
    coded = coded * np.where(coded[:, :1] < 0, -1.0, 1.0)
    assert np.abs(f["rotations"][:, [3, 0, 1, 2]] - coded).max() < 1e-6                 # the fill returns x, y, z, w with w >= 0, fp32
    if ncoef:
        per = ncoef // 3
        r = rest.reshape(N, 3, per)
        coded = np.stack([nearest(r[:, :, k]) for k in range(per)], axis=2)          # [splat, channel, coefficient]
        want = np.concatenate([np.transpose(coded[:, :, lo:hi], (0, 2, 1)).reshape(N, -1) for lo, hi in ((0, 3), (3, 8))[:degree]], axis=1)
        assert np.array_equal(np.asarray(f["sh_f16"]).view(np.float16).astype(np.float64), want)


# ------------------------------------------------------------------------------------------------ damage
WORDS = ["char", "uchar", "short", "ushort", "int", "uint", "float", "double", "list", "property", "element", "comment", "format", "vertex",
         "codebook_centers", "x", "rot_0", "f_rest_3", "f_rest_45", "scaling", "features_rest_2", "opacity", "0", "1", "255", "256", "257",
         "599", "601", "65536", "4294967295", "4294967296", "-3", "end_header", "binary_little_endian", "ascii", ""]


def mutations(count=300, seed=2024):
    """Seeded damage to valid files: header words replaced, element counts changed, header lines dropped or doubled, truncation, and
    random bytes anywhere."""
    rng = np.random.default_rng(seed)
    bases = [v2(0), v2(9, codebook_first=True), v2(24), v2(45, half_type="ushort")]
    out = []
    for k in range(count):
        data = bytearray(bases[k % len(bases)])
        end = data.index(b"end_header\n") + 11
        lines = data[:end].decode().split("\n")[:-1]
        kind = k % 5
        if kind == 0:                                                                 # a header word
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(1, len(lines)))
                words = lines[at].split(" ")
                words[int(rng.integers(0, len(words)))] = WORDS[int(rng.integers(0, len(WORDS)))]
                lines[at] = " ".join(words)
        elif kind == 1:                                                               # an element count
            at = [i for i, line in enumerate(lines) if line.startswith("element")][int(rng.integers(0, 2))]
            words = lines[at].split(" ")
            words[2] = str(int(rng.choice([0, 1, 255, 256, 257, 599, 601, 70000, 2 ** 32 - 1, 2 ** 32, int(rng.integers(0, 2 ** 31))])))
            lines[at] = " ".join(words)
        elif kind == 2:                                                               # a line dropped, doubled or moved
            at = int(rng.integers(1, len(lines)))
            line = lines.pop(at)
            if rng.random() < 0.6:
                lines.insert(int(rng.integers(1, len(lines) + 1)), line)
                if rng.random() < 0.5:
                    lines.insert(at, line)
        if kind <= 2:
            data = bytearray(("\n".join(lines) + "\n").encode()) + data[end:]
        elif kind == 3:                                                               # truncation
            data = data[:int(rng.integers(0, len(data)))]
        else:                                                                         # random bytes, in the header more often than not
            for _ in range(int(rng.integers(1, 20))):
                at = int(rng.integers(0, end if rng.random() < 0.6 else len(data)))
                data[at] = int(rng.integers(0, 256))
        out.append(bytes(data))
    return out


def test_damaged_files_are_refused_or_read():
    """Each of 300 mutated files is refused (`out` left NULL) or opens and fills.  (That no read leaves
    the file is checked by running the same files through a sanitizer build of the reader, outside pytest.)"""
    lib = L.load()
    opened = refused_by_name = 0
    for data in mutations():
        st, handle = open_status(data, L.GS_ASSET_PLY)
        if st != L.GS_OK:
            assert st == L.GS_ERR_INVALID and handle is None
            refused_by_name += b"INRIA-v2 PLY:" in lib.gs_last_error()
            continue
        n, degree, f = opens(data)
        assert degree <= 2 and f["centers"].shape == (n, 3) and f["cov"].shape == (n, 6)
        opened += 1
    assert opened >= 30 and refused_by_name >= 100, (opened, refused_by_name)         # the run reaches both outcomes
