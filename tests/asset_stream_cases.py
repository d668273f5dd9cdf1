"""What tests/test_asset_stream.py (CPU) and tests/test_gpu_asset_stream.py (-m gpu) share: the files a stream is fed - the small
reference-recorded ones under tests/golden/ and seeded ones from the writers of gaussiansplats3d_amd.assets - a model of "how
many splats are ready after how many bytes" computed in Python from each file's layout (never from the library), and the ways
a file is cut into appends."""
import json
import os
import struct

import numpy as np

import asset_formats_cases
import asset_inria_v2_cases
import asset_spz_cases
import ksplat_sections
from gaussiansplats3d_amd import assets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_PLY_SIZE = {"char": 1, "uchar": 1, "short": 2, "ushort": 2, "int": 4, "uint": 4, "float": 4, "double": 8}
_PLY_NP = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4", "double": "<f8"}


# ------------------------------------------------------------------------------------------------ INRIA-v1 files
def v1_inputs(n, n_rest, seed):
    rng = np.random.default_rng(seed)
    return dict(centers=rng.normal(size=(n, 3)).astype(np.float32), log_scales=rng.normal(-4, 1, size=(n, 3)).astype(np.float32),
                rotations=rng.normal(size=(n, 4)).astype(np.float32), f_dc=rng.normal(0, 1.2, size=(n, 3)).astype(np.float32),
                opacity=rng.normal(0, 3, size=n).astype(np.float32),
                f_rest=rng.normal(0, 0.2, size=(n, n_rest)).astype(np.float32) if n_rest else None)


def v1_file(n, n_rest, seed, extra_uchar=False, centers=None):
    c = v1_inputs(n, n_rest, seed)
    if centers is not None:
        c["centers"] = np.asarray(centers, np.float32)
    extra = np.random.default_rng(seed + 1).integers(0, 256, n).astype(np.uint8) if extra_uchar else None
    return assets.write_ply(c["centers"], c["log_scales"], c["rotations"], c["f_dc"], c["opacity"], c["f_rest"], extra)


def packed_ply(props, columns, n):
    """A binary little-endian PLY of one vertex element: props [(type, name)], columns {name: values}."""
    rec = np.zeros(n, dtype=[(nm, _PLY_NP[typ]) for typ, nm in props])
    for nm, v in columns.items():
        rec[nm] = v
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    head += "".join(f"property {typ} {nm}\n" for typ, nm in props) + "end_header\n"
    return head.encode() + rec.tobytes()


def v1_rgb_file(n=257, seed=21, centers=None, opacity=False):
    """No scale_*, opacity or f_dc_*: the red / green / blue branch (uchar, normalised) and the 0.01 default scale.  The stride is
    odd (31 bytes).  Without an opacity every splat is transparent (createSplat starts it at 0); opacity: with one, so that the
    branch also reaches a frame."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 3)) if centers is None else np.asarray(centers)
    q = rng.normal(size=(n, 4))
    props = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue"),
             ("float", "rot_0"), ("float", "rot_1"), ("float", "rot_2"), ("float", "rot_3")]
    cols = {"x": c[:, 0], "y": c[:, 1], "z": c[:, 2], "red": rng.integers(0, 256, n), "green": rng.integers(0, 256, n),
            "blue": rng.integers(0, 256, n), "rot_0": q[:, 0], "rot_1": q[:, 1], "rot_2": q[:, 2], "rot_3": q[:, 3]}
    if opacity:
        props.append(("float", "opacity"))
        cols["opacity"] = rng.normal(2.0, 2.0, size=n)
    return packed_ply(props, cols, n)


def v1_typed_file(n=257, seed=22, centers=None):
    """Mapped fields as short, int, ushort, uint and uchar (PlyParserUtils.readVertex reads each by its type), a double nothing reads
    and fields at odd offsets."""
    rng = np.random.default_rng(seed)
    c = (rng.normal(size=(n, 3)) * 3).round() if centers is None else np.asarray(centers).round()
    props = [("uchar", "pad0"), ("short", "x"), ("int", "y"), ("short", "z"), ("double", "nx"), ("uchar", "scale_0"), ("short", "scale_1"),
             ("int", "scale_2"), ("int", "rot_0"), ("short", "rot_1"), ("uchar", "rot_2"), ("ushort", "rot_3"), ("uchar", "f_dc_0"),
             ("short", "f_dc_1"), ("uint", "f_dc_2"), ("uchar", "opacity")]
    cols = {"pad0": rng.integers(0, 256, n), "x": c[:, 0], "y": c[:, 1], "z": c[:, 2], "nx": rng.normal(size=n),
            "scale_0": rng.integers(0, 256, n), "scale_1": rng.integers(-6, 1, n), "scale_2": rng.integers(-6, 1, n),
            "rot_0": rng.integers(-5, 6, n), "rot_1": rng.integers(-5, 6, n), "rot_2": rng.integers(0, 256, n),
            "rot_3": rng.integers(0, 9, n), "f_dc_0": rng.integers(0, 256, n), "f_dc_1": rng.integers(-2, 3, n),
            "f_dc_2": rng.integers(0, 3, n), "opacity": rng.integers(0, 256, n)}
    return packed_ply(props, cols, n)


def v1_hostile_file(n=257, seed=23, centers=None):
    """Hostile rows among ordinary ones: NaN, +-Inf and denormals in positions, scales, colours and opacity, scale_0 = 89 (e^89
    overflows fp32) and 710 (overflows fp64), opacity +-800, an all-zero and a denormal quaternion.  No NaN / Inf among the rotation
    fields: a NaN that the quaternion arithmetic makes is stored canonical by a stream and with the host's sign by gs_asset_open."""
    c = v1_inputs(n, 9, seed)
    if centers is not None:
        c["centers"] = np.asarray(centers, np.float32)
    den = np.float32(1e-42)
    c["centers"][3] = [np.nan, 0.5, -0.5]
    c["centers"][4] = [np.inf, -np.inf, den]
    c["log_scales"][5] = [89.0, 710.0, -np.inf]
    c["log_scales"][6] = [np.nan, np.inf, den]
    c["log_scales"][7] = [-745.2, -103.9, 88.7]
    c["opacity"][8], c["opacity"][9], c["opacity"][10], c["opacity"][11] = 800.0, -800.0, np.nan, np.inf
    c["opacity"][12], c["opacity"][13] = -np.inf, den
    c["f_dc"][14] = [np.nan, np.inf, -np.inf]
    c["f_dc"][15] = [den, -den, 1e30]
    c["rotations"][16] = 0.0
    c["rotations"][17] = [den, -den, den, 0.0]
    c["f_rest"][18, :4] = [np.nan, np.inf, -np.inf, den]
    return assets.write_ply(c["centers"], c["log_scales"], c["rotations"], c["f_dc"], c["opacity"], c["f_rest"])


NAN_ROTATION_ROWS = [5, 40, 41, 200]


def v1_nan_rotations_file(n=257, seed=24, centers=None):
    """Rows whose rot_* hold an infinity or a NaN (with a sign and a payload): the quaternion's normalisation makes NaNs of them.  Kept
    apart from V1_CASES: here a stream and gs_asset_open agree on where the NaNs are, not on their bits."""
    c = v1_inputs(n, 9, seed)
    if centers is not None:
        c["centers"] = np.asarray(centers, np.float32)
    c["rotations"][5] = [np.inf, 0.1, 0.2, 0.3]
    c["rotations"][40] = [0.5, -np.inf, 0.2, np.inf]
    c["rotations"][41] = np.array([0xFFC12345, 0x3F000000, 0x3F000000, 0x3F000000], np.uint32).view(np.float32)
    c["rotations"][200] = [0.1, 0.2, 0.3, np.nan]
    return assets.write_ply(c["centers"], c["log_scales"], c["rotations"], c["f_dc"], c["opacity"], c["f_rest"])


# (the name, how to make it, the output degree it is opened at): every seeded INRIA-v1 case
V1_CASES = {
    "v1_sh0": (lambda n, c: v1_file(n, 0, 11, centers=c), 2),
    "v1_sh1": (lambda n, c: v1_file(n, 9, 12, centers=c), 2),
    "v1_sh2": (lambda n, c: v1_file(n, 24, 13, centers=c), 2),
    "v1_sh3": (lambda n, c: v1_file(n, 45, 14, centers=c), 2),
    "v1_sh2_at_degree_1": (lambda n, c: v1_file(n, 24, 15, centers=c), 1),
    "v1_odd_stride": (lambda n, c: v1_file(n, 9, 16, extra_uchar=True, centers=c), 2),
    "v1_rgb_no_scale": (lambda n, c: v1_rgb_file(n, centers=c), 2),
    "v1_rgb_with_opacity": (lambda n, c: v1_rgb_file(n, centers=c, opacity=True), 2),
    "v1_typed": (lambda n, c: v1_typed_file(n, centers=c), 2),
    "v1_hostile": (lambda n, c: v1_hostile_file(n, centers=c), 2),
}


def v1_case(name, n=257, centers=None):
    if name == "v1_nan_rotations":
        return v1_nan_rotations_file(n, centers=centers), "ply", 2
    make, degree = V1_CASES[name]
    return make(n, centers), "ply", degree


# ------------------------------------------------------------------------------------------------ all six formats
def _rows(n, seed, ncoef=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)), rng.normal(-3.0, 0.5, size=(n, 3)), rng.normal(size=(n, 4)), rng.random((n, 4)),
            rng.normal(0.0, 0.4, size=(n, ncoef)) if ncoef else None)


def _ref_golden(case, key):
    g = np.load(os.path.join(GOLDEN, f"assets_ref_{case}.npz"))
    man = json.loads(bytes(g["manifest"]).decode())
    return bytes(g[key]), ("ply" if key == "ply_bytes" else "ksplat"), man["shDegree"]


def _make_files():
    """{name: (bytes, fmt, output degree)}"""
    f = {}
    for name in V1_CASES:
        f[name] = v1_case(name, 257 if name != "v1_sh0" else 64)
    for case in ("sh0", "sh2"):                                                 # reference-written INRIA-v1 and .ksplat files
        f[f"ref_{case}_ply"] = _ref_golden(case, "ply_bytes")
        for lvl in (0, 1, 2):
            f[f"ref_{case}_gen{lvl}"] = _ref_golden(case, f"gen{lvl}_ksplat")
    for mod, tag in ((asset_formats_cases, "fmt"), (asset_spz_cases, "spz"), (asset_inria_v2_cases, "iv2")):
        for name in mod.cases()[:3]:
            data, fmt, degree, _ = mod.case(name)
            f[f"{tag}_{name}"] = (data, fmt, degree)
    c, ls, q, rgba, _ = _rows(300, 31)
    f["splat_300"] = (assets.write_splat(c, np.exp(ls), q, (rgba * 255).astype(np.uint8)), "splat", 0)
    for ncoef, degree in ((0, 2), (9, 2), (24, 2), (24, 0)):                    # 600 splats: two full chunks and one of 88
        c, ls, q, rgba, sh = _rows(600, 32 + ncoef, ncoef)
        f[f"pc_{ncoef}_at_{degree}"] = (assets.write_compressed_ply(c, ls, q, rgba, sh, color_extremes=ncoef == 9), "ply", degree)
    for level, degrees in ((0, (1, 2)), (1, (1, 1)), (2, (2, 1))):              # 301 splats, an empty section, 310 splats
        f[f"ksplat_l{level}_3sec"] = (ksplat_sections.three_sections(level, degrees), "ksplat", 2)
    c, ls, q, rgba, sh = _rows(300, 41, 9)
    f["spz_300"] = (assets.write_spz(c, ls, q, rgba, sh), "spz", 2)
    f["iv2_300"] = (assets.write_inria_v2_ply(c, ls, q, rgba[:, :3], rgba[:, 3], sh), "ply", 2)
    f["iv2_300_codebook_first"] = (assets.write_inria_v2_ply(c, ls, q, rgba[:, :3], rgba[:, 3], sh, codebook_first=True), "ply", 2)
    return f


_FILES = {}


def files():
    if not _FILES:
        _FILES.update(_make_files())
    return _FILES


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """How far a stream of `data` is after `received` bytes, from the file's layout alone.
    header_at: the byte count at which header_ready flips (None: only with the final append).
    runs: [(gate, rows_off, stride, count)] in file order.  borders: byte offsets worth cutting at."""

    def __init__(self, data, fmt, degree):
        self.size, self.header_at, self.runs, self.borders = len(data), None, [], []
        if fmt == "splat":
            self.header_at, self.runs = 0, [(0, 0, 32, len(data) // 32)]
            self.borders = [32, 32 * (len(data) // 64)]
        elif fmt == "ksplat":
            self._ksplat(data)
        elif fmt == "ply":
            self._ply(data, degree)
        self.count = sum(r[3] for r in self.runs)

    def _ksplat(self, data):
        sections = struct.unpack_from("<I", data, 4)[0]
        level = struct.unpack_from("<H", data, 20)[0]
        self.header_at = 4096 + 1024 * sections
        self.borders = [4096, self.header_at]
        base = self.header_at
        for s in range(sections):
            h = 4096 + 1024 * s
            count, _, bucket_count = struct.unpack_from("<III", data, h + 4)
            storage = struct.unpack_from("<H", data, h + 20)[0]
            partial = struct.unpack_from("<I", data, h + 36)[0]
            sh = {0: 0, 1: 9, 2: 24}[struct.unpack_from("<H", data, h + 40)[0]]
            bps = [44, 24, 24][level] + [4, 2, 1][level] * sh
            rows = base + 4 * partial + storage * bucket_count
            if count:
                self.runs.append((rows, rows, bps, count))
            self.borders += [base + 4 * partial, rows, rows + bps]
            base = rows + bps * count
            self.borders.append(base)

    def _ply(self, data, degree):
        end = data.index(b"end_header\n") + 11
        lines = data[:end].decode().split("\n")
        elements = []
        for line in lines:
            w = line.split()
            if w[:1] == ["element"]:
                elements.append([w[1], int(w[2]), 0])
            elif w[:1] == ["property"]:
                elements[-1][2] += _PLY_SIZE[w[1]]
        names = [e[0] for e in elements]
        self.borders = [end]
        off = end
        bases = {}
        for name, count, stride in elements:
            bases[name] = (off, count, stride)
            off += count * stride
            self.borders += [bases[name][0] + stride, off]
        if "codebook_centers" in names:                      # INRIA-v2: nothing before the end
            return
        self.header_at = end
        if "chunk" in names:                                 # compressed: the chunk element gates; above degree 0 the SH row counts
            v0, n, _ = bases["vertex"]
            file_degree = {0: 0, 9: 1, 24: 2, 45: 2}[bases["sh"][2]] if "sh" in bases else 0
            if min(degree, file_degree) > 0:
                self.runs = [(v0, bases["sh"][0], bases["sh"][2], n)]
            else:
                self.runs = [(v0, v0, 16, n)]
        else:
            v0, n, stride = bases["vertex"]
            self.runs = [(v0, v0, stride, n)]

    def at(self, received, final=False):
        """(header_ready, splats_ready)"""
        if final:
            return True, None                                # all: the caller knows the whole file's count
        ready = 0
        for gate, rows_off, stride, count in self.runs:
            if received < gate or received < rows_off:
                break
            rows = min(count, (received - rows_off) // stride)
            ready += rows
            if rows < count:
                break
        return self.header_at is not None and received >= self.header_at, ready


# ------------------------------------------------------------------------------------------------ cutting a file into appends
def by_size(total, size):
    return list(range(size, total, size)) + [total]


def around(total, borders):
    """Cut points at every border - 1 / 0 / + 1."""
    pts = sorted({p + d for p in borders for d in (-1, 0, 1) if 0 < p + d < total})
    return pts + [total]


def feed(stream, data, ends):
    """Appends data[.. ends[0]], data[ends[0] .. ends[1]], ...; the last with final.  Yields (bytes so far, is final, stream_info)."""
    at = 0
    for k, end in enumerate(ends):
        final = k == len(ends) - 1
        info = stream.append(data[at:end], final)
        at = end
        yield at, final, info
