"""Host-side mirror of the reference's scene loaders, over the native readers of libgsplat_hip (csrc/assets.hip).

Reference interface: ``PlyLoader.loadFromFileData`` / ``KSplatLoader.loadFromFileData`` / ``SplatLoader`` /
``SpzLoader.loadFromFileData`` -> ``SplatBuffer``
(/root/reference/src/loaders/ply/PlyLoader.js, src/loaders/ksplat/KSplatLoader.js, src/loaders/splat/SplatLoader.js's
progressive file-order path, src/loaders/spz/SpzLoader.js with ``optimizeSplatData: false``) followed by
``SplatMesh.fillSplatDataArrays`` (src/splatmesh/SplatMesh.js:1853-1902), with the scene's static transform when
``SplatAsset.set_transform`` gave one.  ``load`` returns the arrays
``SplatMesh.build`` / the sort worker take.  ``"ply"`` covers INRIA-v1, the PlayCanvas / SuperSplat compressed PLY and the INRIA-v2
codebook PLY of the "reduced 3DGS" trainer (src/loaders/ply/INRIAV2PlyParser.js, kept in file order; decided from the header);
``"splat"`` has no magic number and is chosen by ``fmt`` or a file name's extension; ``"spz"`` is a gzip
member (``1f 8b``), inflated by the library itself, and is chosen by ``fmt``, the extension or that magic.  The ``write_*``
helpers produce the same file formats (used by the tests and to stage synthetic scenes as real files); they are not part
of the reference's API surface.
"""
import ctypes as C
import gzip
import struct

import numpy as np

from . import _lib as L
from .util import to_half_three


class SplatAsset:
    """An opened .ply / .ksplat / .splat / .spz: ``info`` + ``fill()`` -> dict of arrays."""
    FORMATS = {"ply": L.GS_ASSET_PLY, "ksplat": L.GS_ASSET_KSPLAT, "splat": L.GS_ASSET_SPLAT, "spz": L.GS_ASSET_SPZ}

    def __init__(self, data, fmt=None, spherical_harmonics_degree=2):
        self.lib = L.load()
        data = bytes(data)
        if fmt is None:
            fmt = "ply" if data[:3] == b"ply" else ("spz" if data[:2] == b"\x1f\x8b" else "ksplat")
        self.handle = C.c_void_p()
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        if fmt not in self.FORMATS:
            raise ValueError(f"unknown asset format {fmt!r}: one of {sorted(self.FORMATS)}")
        if fmt == "spz" and data[:2] != b"\x1f\x8b":
            raise ValueError("not an .spz file: the data does not start with the gzip magic 1f 8b")
        L.check(self.lib.gs_asset_open(buf, len(data), self.FORMATS[fmt], int(spherical_harmonics_degree), C.byref(self.handle)))
        self.info = L.AssetInfo()
        L.check(self.lib.gs_asset_get_info(self.handle, C.byref(self.info)))

    def set_transform(self, matrix):
        """The static-mode scene transform (gs_asset_set_transform): 16 numbers, column-major like
        ``THREE.Matrix4.elements`` (a 4x4 array is read as elements[4 * column + row]), or None to remove it.  ``fill``,
        ``upload_to`` and ``upload_centers_to`` then return what the reference's fills return with that transform; an
        identity matrix is not the same as None for the SH of a level-2 file."""
        if matrix is None:
            L.check(self.lib.gs_asset_set_transform(self.handle, None))
            return
        m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).reshape(-1))
        if m.size != 16:
            raise ValueError("a scene transform has 16 elements")
        L.check(self.lib.gs_asset_set_transform(self.handle, m.ctypes.data))

    def fill(self, minimum_alpha=1, half_precision_covariances=False, want_scale_rotation=False):
        n, deg = self.info.splat_count, self.info.sh_degree
        ncoef = {0: 0, 1: 9, 2: 24}[deg]
        out = {"centers": np.empty((n, 3), np.float32), "rgba": np.empty((n, 4), np.uint8), "sh_degree": deg,
               "sh_level": self.info.sh_level, "sh_range": (self.info.sh_min, self.info.sh_max)}
        cov32 = None if half_precision_covariances else np.empty((n, 6), np.float32)
        cov16 = np.empty((n, 6), np.uint16) if half_precision_covariances else None
        sh16 = np.empty((n, ncoef), np.uint16) if (ncoef and self.info.sh_level == 1) else None
        sh8 = np.empty((n, ncoef), np.uint8) if (ncoef and self.info.sh_level == 2) else None
        sc = np.empty((n, 3), np.float32) if want_scale_rotation else None
        ro = np.empty((n, 4), np.float32) if want_scale_rotation else None
        p = lambda a: a.ctypes.data if a is not None else None      # noqa: E731
        L.check(self.lib.gs_asset_fill(self.handle, int(minimum_alpha), p(out["centers"]), p(cov32), p(cov16), p(out["rgba"]),
                                       p(sh16), p(sh8), p(sc), p(ro)))
        out.update(cov=cov32, cov_f16=cov16, sh_f16=sh16, sh_u8=sh8, scales=sc, rotations=ro)
        return out

    def upload_to(self, mesh, frm=0, first=0, count=None, minimum_alpha=1):
        """Decode splats [first, first + count) on the device into splats [frm, frm + count) of ``mesh``
        (gs_mesh_upload_asset): what ``fill()`` + ``SplatMesh.build`` / ``update_data`` of the range leave, without the
        decoded arrays ever existing on the host."""
        count = self.info.splat_count - first if count is None else count
        L.check(self.lib.gs_mesh_upload_asset(mesh.handle, int(frm), self.handle, int(first), int(count), int(minimum_alpha)))
        mesh.splat_count = max(mesh.splat_count, int(frm) + int(count))

    def upload_centers_to(self, sorter, frm=0, first=0, count=None, scene_indexes=None):
        """The sort worker's ``centers`` message for the same range, derived on the device
        (gs_sorter_upload_asset_centers): integer or float centres as the worker was created."""
        count = self.info.splat_count - first if count is None else count
        scene = None
        if sorter.dynamic_mode:
            scene = np.ascontiguousarray(scene_indexes, dtype=np.uint32).reshape(-1)
            if scene.size != count:
                raise ValueError("scene_indexes must hold one index per splat of the range")
        L.check(self.lib.gs_sorter_upload_asset_centers(sorter.handle, int(frm), self.handle, int(first), int(count),
                                                        scene.ctypes.data if scene is not None else None))
        sorter.uploaded_splat_count = max(sorter.uploaded_splat_count, int(frm) + int(count))

    def encode_ksplat(self, ctx, compression_level=1, minimum_alpha=1, block_size=5.0, bucket_size=256, scene_center=(0, 0, 0)):
        """This asset as a one-section .ksplat, encoded on the device (gs_asset_encode_ksplat): byte for byte what
        ``SplatBuffer.generateFromUncompressedSplatArrays`` returns for the asset's level-0 rows in file order
        (/root/reference/src/loaders/SplatBuffer.js:1177-1326; util/create-ksplat.js without its partitioner).  Returns
        ``(SplatAsset, order)``: the opened result (``to_bytes()`` is the file) and, per output position, the index of the
        source splat stored there."""
        p = L.KsplatParams(int(compression_level), int(minimum_alpha), int(bucket_size), float(block_size),
                           (C.c_float * 3)(*[float(v) for v in scene_center]), 0)
        order = np.empty(self.info.splat_count, np.uint32)
        handle = C.c_void_p()
        L.check(self.lib.gs_asset_encode_ksplat(ctx.handle if ctx is not None else None, self.handle, C.byref(p), C.byref(handle),
                                                order.ctypes.data))
        out = SplatAsset.__new__(SplatAsset)
        out.lib, out.handle, out.info = self.lib, handle, L.AssetInfo()
        L.check(self.lib.gs_asset_get_info(handle, C.byref(out.info)))
        return out, order[:out.info.splat_count].copy()

    def to_bytes(self):
        """The file image of an ``encode_ksplat`` result (gs_asset_bytes)."""
        data, size = C.c_void_p(), C.c_uint64()
        L.check(self.lib.gs_asset_bytes(self.handle, C.byref(data), C.byref(size)))
        return C.string_at(data, size.value)

    def close(self):
        if self.handle:
            self.lib.gs_asset_close(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SplatAssetStream(SplatAsset):
    """An asset handed over as it arrives (gs_asset_open_stream): ``append(data, final)`` takes the next piece, and after
    every append ``upload_to`` / ``upload_centers_to`` take any range of the first ``stream_info.splats_ready`` splats - a
    prefix of the whole file's numbering that never shrinks.  Once the final append is accepted it is the ``SplatAsset`` of
    the concatenated bytes: ``fill`` and ``encode_ksplat`` work from then on (gsplat_hip.h: rules M and P).  ``fmt`` is
    required (a stream has no bytes to look at); ``"splat"`` needs ``expected_bytes``.  ``info`` is None until the header is in.
    The appends and uploads of one stream come from one thread."""

    def __init__(self, fmt, spherical_harmonics_degree=2, expected_bytes=0):
        self.lib = L.load()
        self.handle = C.c_void_p()
        self.info = None
        if fmt not in self.FORMATS:
            raise ValueError(f"unknown asset format {fmt!r}: one of {sorted(self.FORMATS)}")
        L.check(self.lib.gs_asset_open_stream(self.FORMATS[fmt], int(spherical_harmonics_degree), int(expected_bytes),
                                              C.byref(self.handle)))
        self._refresh()

    def _refresh(self):
        info = self.stream_info
        if info.header_ready:
            self.info = L.AssetInfo()
            L.check(self.lib.gs_asset_get_info(self.handle, C.byref(self.info)))
        return info

    @property
    def stream_info(self):
        info = L.AssetStreamInfo()
        L.check(self.lib.gs_asset_get_stream_info(self.handle, C.byref(info)))
        return info

    def append(self, data, final=False):
        """The next piece of the file (any length, empty too); ``final`` with the last one.  Returns ``stream_info``.  A
        refused append raises, consumes nothing and ends the stream; what was ready stays uploadable."""
        data = bytes(data)
        L.check(self.lib.gs_asset_append(self.handle, data, len(data), int(bool(final))))
        return self._refresh()

    def upload_to(self, mesh, frm=0, first=0, count=None, minimum_alpha=1):
        count = self.stream_info.splats_ready - first if count is None else count
        super().upload_to(mesh, frm, first, count, minimum_alpha)

    def upload_centers_to(self, sorter, frm=0, first=0, count=None, scene_indexes=None):
        count = self.stream_info.splats_ready - first if count is None else count
        super().upload_centers_to(sorter, frm, first, count, scene_indexes)


def load(path_or_bytes, spherical_harmonics_degree=2, minimum_alpha=1, half_precision_covariances=False):
    fmt = None
    if isinstance(path_or_bytes, str):
        if path_or_bytes.lower().endswith(".splat"):          # .splat has no magic number: the extension decides
            fmt = "splat"
        elif path_or_bytes.lower().endswith(".spz"):
            fmt = "spz"
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    else:
        data = path_or_bytes
    a = SplatAsset(data, fmt, spherical_harmonics_degree)
    try:
        return a.fill(minimum_alpha, half_precision_covariances)
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------ writers
def write_ply(centers, log_scales, rotations_wxyz, f_dc, opacity_logit, f_rest=None, extra_uchar=None):
    """INRIA-v1 layout: x y z [nx ny nz] f_dc_0..2 f_rest_* opacity scale_0..2 rot_0..3, float32 little endian.
    f_rest: [n, 3*cpc] channel-major as the INRIA trainer writes it (all R coefficients, then G, then B)."""
    n = centers.shape[0]
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    cols = [centers[:, 0], centers[:, 1], centers[:, 2], np.zeros(n), np.zeros(n), np.zeros(n), f_dc[:, 0], f_dc[:, 1], f_dc[:, 2]]
    if f_rest is not None:
        for k in range(f_rest.shape[1]):
            names.append(f"f_rest_{k}")
            cols.append(f_rest[:, k])
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    cols += [opacity_logit, log_scales[:, 0], log_scales[:, 1], log_scales[:, 2], rotations_wxyz[:, 0], rotations_wxyz[:, 1],
             rotations_wxyz[:, 2], rotations_wxyz[:, 3]]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {nm}\n" for nm in names)
    if extra_uchar is not None:
        header += "property uchar pad\n"
    header += "end_header\n"
    body = np.stack([np.asarray(c, np.float32) for c in cols], axis=1)
    if extra_uchar is None:
        return header.encode() + np.ascontiguousarray(body).tobytes()
    rec = np.zeros(n, dtype=[("f", np.float32, body.shape[1]), ("u", np.uint8)])
    rec["f"], rec["u"] = body, extra_uchar
    return header.encode() + rec.tobytes()


def write_splat(centers, scales, rotations_wxyz, rgba):
    """.splat rows (src/loaders/splat/SplatParser.js:77-82): centre 3 x f32, scale 3 x f32 (linear), RGBA 4 x u8, rotation
    4 x u8 as round(q / |q| * 128 + 128) clipped to 0..255, stored w, x, y, z."""
    n = centers.shape[0]
    q = np.asarray(rotations_wxyz, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    rec = np.zeros(n, dtype=[("c", "<f4", 3), ("s", "<f4", 3), ("rgba", np.uint8, 4), ("rot", np.uint8, 4)])
    rec["c"], rec["s"], rec["rgba"] = centers, scales, np.asarray(rgba, np.uint8).reshape(n, 4)
    rec["rot"] = np.clip(np.floor(q * 128 + 128 + 0.5), 0, 255).astype(np.uint8)
    return rec.tobytes()


def spz_stream(centers, log_scales, rotations, rgba, sh=None, version=2, fractional_bits=12, sh_degree=None):
    """The uncompressed .spz stream ``write_spz`` wraps in gzip: the 16-byte header and the six planes."""
    n = centers.shape[0]
    dims = {0: 0, 1: 3, 2: 8, 3: 15}
    if sh_degree is None:
        sh_degree = 0 if sh is None else {9: 1, 24: 2, 45: 3}[np.asarray(sh).reshape(n, -1).shape[1]]
    dim = dims[sh_degree]
    c = np.asarray(centers, np.float64)
    if version == 2:
        fixed = np.clip(np.floor(c * float(1 << fractional_bits) + 0.5), -(1 << 23), (1 << 23) - 1).astype(np.int64) & 0xFFFFFF
        positions = np.stack([(fixed >> s) & 255 for s in (0, 8, 16)], axis=2).astype(np.uint8).tobytes()     # [n, 3 axes, 3 bytes]
    else:
        positions = c.astype("<f2").tobytes()
    rgba = np.asarray(rgba, np.float64).reshape(n, 4)
    u8 = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)                                   # noqa: E731
    q = np.asarray(rotations, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q = q * np.where(q[:, :1] < 0, -1.0, 1.0)                       # w is rebuilt as a non-negative root
    planes = [positions, u8(rgba[:, 3] * 255).tobytes(),
              u8(((rgba[:, :3] - 0.5) / 0.28209479177387814 * 0.15 + 0.5) * 255).tobytes(),
              u8((np.asarray(log_scales, np.float64) + 10.0) * 16.0).tobytes(), u8((q[:, 1:] + 1.0) * 127.5).tobytes()]
    if dim:
        s = np.asarray(sh, np.float64).reshape(n, 3, dim)           # [splat, channel, coefficient] -> coefficient-major on the wire
        planes.append(u8(np.transpose(s, (0, 2, 1)) * 128.0 + 128.0).tobytes())
    header = struct.pack("<IIIBBBB", 1347635022, version, n, sh_degree, fractional_bits, 0, 0)
    return header + b"".join(planes)


def write_spz(centers, log_scales, rotations, rgba, sh=None, version=2, fractional_bits=12, sh_degree=None):
    """.spz (src/loaders/spz/SpzLoader.js:255-342), a quantising writer: a gzip member around the 16-byte header and the
    planes positions (version 2: 24-bit fixed point with ``fractional_bits``; version 1: halves), alphas, colours
    (``((c - 0.5) / SH_C0 * 0.15 + 0.5) * 255``: the inverse of the reader's rule), scales (``(log + 10) * 16``), rotations
    (x, y, z of the unit quaternion with w >= 0 as ``(v + 1) * 127.5``) and SH (``v * 128 + 128``).  rotations: w, x, y, z;
    rgba: floats in 0..1 [n, 4]; sh: float [n, 9|24|45] in the file order of the other writers (all R coefficients, then
    G, then B); sh_degree defaults to what ``sh`` holds."""
    return gzip.compress(spz_stream(centers, log_scales, rotations, rgba, sh, version, fractional_bits, sh_degree), 6, mtime=0)


_PLY_NP = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4", "double": "<f8"}


def _codebook_page(values):
    """256 half-float entries at the quantiles of ``values`` and, per value, the index of the nearest entry."""
    v = np.asarray(values, np.float64).reshape(-1)
    finite = v[np.isfinite(v)]
    finite = finite[::max(1, finite.size >> 20)]                    # a million values place the quantiles of a large scene
    entries = np.sort(np.quantile(finite if finite.size else np.zeros(1), (np.arange(256) + 0.5) / 256).astype(np.float16))
    e = entries.astype(np.float64)
    index = np.searchsorted((e[:-1] + e[1:]) / 2, np.where(np.isfinite(v), v, 0.0)).astype(np.uint8)
    return entries, index.reshape(np.shape(values))


def write_inria_v2_ply(centers, log_scales, rotations_wxyz, f_dc, opacity_logit, f_rest=None, codebook_first=False, half_type="short",
                       extra_vertex=None, extra_codebook=None, field_order=None, comment=None, codebook_override=None,
                       index_override=None):
    """INRIA-v2 codebook PLY (src/loaders/ply/INRIAV2PlyParser.js), a quantising writer: x y z as half floats, every other
    attribute as one uchar index into a 256-entry page of the `codebook_centers` element (half floats too; halves are stored as
    16-bit integers of ``half_type`` "short" / "ushort", as the trainer stores them).  The pages: features_dc (the three f_dc_*
    share it), features_rest_k (coefficient k of all three channels), opacity, scaling (log scales), rotation_re (rot_0) and
    rotation_im (rot_1..3); each holds the quantiles of its data, and a value is coded as its nearest entry.
    log_scales / f_dc / opacity_logit may be None: the file then lacks those fields.  f_rest: [n, 9|24|45] channel-major as the
    trainer writes it.  codebook_first: the codebook element precedes the vertex element.  extra_vertex / extra_codebook:
    [(type, name)] properties nothing reads.  field_order: a permutation of the vertex property names.  codebook_override:
    {page: {entry: value}} replaces entries after the indexes were chosen, {page: None} leaves the page out; index_override:
    {field: {row: index}}."""
    n = centers.shape[0]
    q = np.asarray(rotations_wxyz, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    pages, fields = {}, [(nm, half_type, np.asarray(centers, np.float64)[:, k].astype(np.float16).view(np.uint16)) for k, nm in enumerate("xyz")]

    def group(page, names, values):
        pages[page], index = _codebook_page(values)
        fields.extend((nm, "uchar", index[:, k]) for k, nm in enumerate(names))

    if f_dc is not None:
        group("features_dc", ["f_dc_0", "f_dc_1", "f_dc_2"], np.asarray(f_dc).reshape(n, 3))
    else:
        pages["features_dc"] = _codebook_page(np.zeros(1))[0]
    if f_rest is not None:
        rest = np.asarray(f_rest, np.float64).reshape(n, 3, -1)                      # [splat, channel, coefficient]
        cpc = rest.shape[2]
        at = len(fields)
        for k in range(cpc):
            group(f"features_rest_{k}", [f"f_rest_{k + cpc * ch}" for ch in range(3)], rest[:, :, k])
        fields[at:] = sorted(fields[at:], key=lambda f: int(f[0][7:]))              # f_rest_0 .. f_rest_{3 cpc - 1} in the row
    for page, names, values in (("opacity", ["opacity"], opacity_logit), ("scaling", ["scale_0", "scale_1", "scale_2"], log_scales)):
        if values is not None:
            group(page, names, np.asarray(values).reshape(n, len(names)))
        else:
            pages[page] = _codebook_page(np.zeros(1))[0]
    group("rotation_re", ["rot_0"], q[:, :1])
    group("rotation_im", ["rot_1", "rot_2", "rot_3"], q[:, 1:])
    for page, edits in (codebook_override or {}).items():
        if edits is None:
            del pages[page]
        else:
            for entry, value in edits.items():
                pages[page][entry] = value
    for k, (typ, nm) in enumerate(extra_vertex or []):
        fields.append((nm, typ, (np.arange(n) % 251 + k).astype(_PLY_NP[typ])))
    if field_order is not None:
        assert sorted(field_order) == sorted(f[0] for f in fields)
        fields = [next(f for f in fields if f[0] == nm) for nm in field_order]
    book = [(nm, half_type, v.view(np.uint16)) for nm, v in pages.items()]
    for k, (typ, nm) in enumerate(extra_codebook or []):
        book.append((nm, typ, (np.arange(256) % 251 + k).astype(_PLY_NP[typ])))

    def element(name, count, props):
        rec = np.zeros(count, dtype=[(nm, _PLY_NP[typ]) for nm, typ, _ in props])
        for nm, typ, v in props:
            rec[nm] = np.asarray(v).view(_PLY_NP[typ]) if typ in ("short", "ushort") else v      # half bits under either name
        for nm, rows in (index_override or {}).items():
            if nm in rec.dtype.names:
                for row, value in rows.items():
                    rec[nm][row] = value
        return f"element {name} {count}\n" + "".join(f"property {typ} {nm}\n" for nm, typ, _ in props), rec.tobytes()

    parts = [element("vertex", n, fields), element("codebook_centers", 256, book)]
    if codebook_first:
        parts.reverse()
    header = "ply\nformat binary_little_endian 1.0\n" + (f"comment {comment}\n" if comment else "")
    return (header + parts[0][0] + parts[1][0] + "end_header\n").encode() + parts[0][1] + parts[1][1]


def pack_unit_quaternions(rotations_wxyz):
    """The 2 + 10 + 10 + 10 rotation word of the compressed PLY: the largest component (by magnitude, made positive) is
    dropped, its index goes to the top two bits, the other three follow in w, x, y, z order scaled by sqrt(2) / 2 into 10 bits."""
    q = np.asarray(rotations_wxyz, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    n = q.shape[0]
    largest = np.argmax(np.abs(q), axis=1)
    q = q * np.where(q[np.arange(n), largest] < 0, -1.0, 1.0)[:, None]
    keep = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[largest]
    rest = np.take_along_axis(q, keep, axis=1)
    u = np.clip(np.floor((rest * (np.sqrt(2) * 0.5) + 0.5) * 1023 + 0.5), 0, 1023).astype(np.uint32)
    return (largest.astype(np.uint32) << 30) | (u[:, 0] << 20) | (u[:, 1] << 10) | u[:, 2]


_PC_CHUNK = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
             "max_scale_x", "max_scale_y", "max_scale_z"]
_PC_COLOR = ["min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]


def write_compressed_ply(centers, log_scales, rotations, rgba, sh=None, color_extremes=False, chunk_order=None, comment=None,
                         rotation_words=None):
    """PlayCanvas / SuperSplat compressed PLY (src/loaders/ply/PlayCanvasCompressedPlyParser.js): chunks of 256 splats with
    fp32 extremes, 11/10/11-bit positions and log scales, 2+10+10+10 rotations of real unit quaternions (w, x, y, z), 8888
    colours, and an `sh` element of one byte per coefficient.  rgba: floats in 0..1 [n, 4] (with color_extremes the colour
    is lerped between per-chunk extremes, min_r .. max_b).  sh: float [n, 9|24|45] in the file's order (all R
    coefficients, then G, then B), coded as round((v + 4) / 8 * 255).  chunk_order: a permutation of the chunk element's
    property names; comment: a `comment` header line; rotation_words: {splat: uint32} overrides."""
    n = centers.shape[0]
    nchunk = (n + 255) // 256
    chunk_of = np.arange(n) // 256
    rgba = np.asarray(rgba, np.float64).reshape(n, 4)

    def extremes(v):
        starts = np.arange(0, n, 256)
        return np.minimum.reduceat(v, starts, axis=0).astype(np.float32), np.maximum.reduceat(v, starts, axis=0).astype(np.float32)

    def unorm(v, lo, hi, bits):
        lo, hi = lo.astype(np.float64)[chunk_of], hi.astype(np.float64)[chunk_of]
        span = np.where(hi > lo, hi - lo, 1.0)
        t = np.clip((v - lo) / span, 0.0, 1.0)
        return np.floor(t * ((1 << bits) - 1) + 0.5).astype(np.uint32)

    def pack111011(v, lo, hi):
        return (unorm(v[:, 0], lo[:, 0], hi[:, 0], 11) << 21) | (unorm(v[:, 1], lo[:, 1], hi[:, 1], 10) << 11) | \
            unorm(v[:, 2], lo[:, 2], hi[:, 2], 11)

    c64, s64 = np.asarray(centers, np.float64), np.asarray(log_scales, np.float64)
    plo, phi = extremes(c64)
    slo, shi = extremes(s64)
    cols = {nm: a[:, k] for nm, a, k in zip(_PC_CHUNK, [plo] * 3 + [phi] * 3 + [slo] * 3 + [shi] * 3, [0, 1, 2] * 4)}
    names = list(_PC_CHUNK)
    if color_extremes:
        clo, chi = extremes(rgba[:, :3])
        cols.update({nm: a[:, k] for nm, a, k in zip(_PC_COLOR, [clo] * 3 + [chi] * 3, [0, 1, 2] * 2)})
        names += _PC_COLOR
        rgb = np.stack([unorm(rgba[:, k], clo[:, k], chi[:, k], 8) for k in range(3)], axis=1)
    else:
        rgb = np.floor(np.clip(rgba[:, :3], 0, 1) * 255 + 0.5).astype(np.uint32)
    alpha = np.floor(np.clip(rgba[:, 3], 0, 1) * 255 + 0.5).astype(np.uint32)
    if chunk_order is not None:
        assert sorted(chunk_order) == sorted(names)
        names = list(chunk_order)
    vertex = np.zeros((n, 4), np.uint32)
    vertex[:, 0] = pack111011(c64, plo, phi)
    vertex[:, 1] = pack_unit_quaternions(rotations)
    for i, word in (rotation_words or {}).items():
        vertex[i, 1] = word
    vertex[:, 2] = pack111011(s64, slo, shi)
    vertex[:, 3] = (rgb[:, 0] << 24) | (rgb[:, 1] << 16) | (rgb[:, 2] << 8) | alpha
    header = "ply\nformat binary_little_endian 1.0\n"
    if comment:
        header += f"comment {comment}\n"
    header += f"element chunk {nchunk}\n" + "".join(f"property float {nm}\n" for nm in names)
    header += f"element vertex {n}\n" + "".join(f"property uint packed_{nm}\n" for nm in ("position", "rotation", "scale", "color"))
    body = np.stack([cols[nm] for nm in names], axis=1).astype("<f4").tobytes() + vertex.astype("<u4").tobytes()
    if sh is not None:
        sh = np.asarray(sh, np.float64).reshape(n, -1)
        header += f"element sh {n}\n" + "".join(f"property uchar f_rest_{k}\n" for k in range(sh.shape[1]))
        body += np.clip(np.floor((sh + 4.0) / 8.0 * 255.0 + 0.5), 0, 255).astype(np.uint8).tobytes()
    return (header + "end_header\n").encode() + body


def write_ksplat(centers, scales, rotations_wxyz, rgba, sh_rows=None, sh_degree=0, compression_level=0, block_size=5.0,
                 bucket_size=256, sh_range=(-1.5, 1.5), scene_center=(0.0, 0.0, 0.0)):
    """One-section .ksplat following SplatBuffer.generateFromUncompressedSplatArrays / writeSplatDataToSectionBuffer
    (src/loaders/SplatBuffer.js:1056-1180, 1182-1320): level 0 = fp32 rows; levels 1/2 = uint16 bucket-relative centres,
    fp16 scale / rotation, fp16 or uint8 SH, buckets of `bucket_size` splats per `block_size`^3 block (splats are
    re-ordered bucket by bucket, like the reference).  sh_rows: float [n, 9|24] in FILE order (per degree: all R, all G,
    all B coefficients).  Returns (bytes, order) with order[k] = input row stored at position k."""
    n = centers.shape[0]
    ncomp = {0: 0, 1: 9, 2: 24}[sh_degree]
    lvl = compression_level
    bps = [44, 24, 24][lvl] + [4, 2, 1][lvl] * ncomp
    c64 = centers.astype(np.float64)
    order = np.arange(n)
    buckets_meta = b""
    n_buckets = full = 0
    partial_lengths = []
    bucket_centers = np.zeros((0, 3), np.float32)
    scale_range = 32767
    if lvl >= 1 and n:
        mn = c64.min(axis=0)
        dims = c64.max(axis=0) - mn
        yb, zb = int(np.ceil(dims[1] / block_size)), int(np.ceil(dims[2] / block_size))
        blk = np.floor((c64 - mn) / block_size).astype(np.int64)
        ids = blk[:, 0] * (yb * zb) + blk[:, 1] * zb + blk[:, 2]
        # A block's splats fill its open bucket in input order; a bucket that reaches bucket_size is closed.  Full buckets are
        # listed in the order they closed, then the open ones by block id (`for (bucketId in obj)`: ascending integer keys).
        by_block = np.argsort(ids, kind="stable")
        sid = ids[by_block]
        starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
        counts = np.diff(np.r_[starts, n])
        rank = np.arange(n) - np.repeat(starts, counts)                     # position of a splat inside its block
        chunk = rank // bucket_size
        is_full = (chunk + 1) * bucket_size <= np.repeat(counts, counts)
        first_of = np.flatnonzero(rank % bucket_size == 0)                  # (in by_block order) first splat of every bucket
        lengths = np.diff(np.r_[first_of, n])
        full_b = is_full[first_of]
        closed_at = by_block[first_of + lengths - 1]                        # input index of the splat that closed the bucket
        key = np.where(full_b, closed_at, n + sid[first_of])               # fulls by closing time, then partials by block id
        blist = np.argsort(key, kind="stable")
        full, n_buckets = int(full_b.sum()), len(first_of)
        partial_lengths = lengths[blist][full:].tolist()
        pos = np.repeat(first_of[blist], lengths[blist]) + (np.arange(n) - np.repeat(np.cumsum(lengths[blist]) - lengths[blist],
                                                                                    lengths[blist]))
        order = by_block[pos].astype(np.int64)
        bucket_centers = blk[by_block[first_of[blist]]] * block_size + mn + block_size / 2.0
        bucket_of = np.repeat(np.arange(n_buckets), lengths[blist])
        buckets_meta = np.array(partial_lengths, np.uint32).tobytes() + bucket_centers.astype(np.float32).tobytes()
    q = rotations_wxyz.astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)                       # tempRot.normalize()
    sf = scale_range / (block_size * 0.5)
    table = np.zeros((n, bps), np.uint8)
    put = lambda col, a: table.__setitem__((slice(None), slice(col, col + a.shape[1] * a.itemsize)),              # noqa: E731
                                           np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)) if n else None
    if lvl == 0:
        put(0, c64[order].astype(np.float32))
        put(12, np.asarray(scales, np.float64)[order].astype(np.float32))
        put(24, q[order].astype(np.float32))
    elif n:
        d = c64[order] - bucket_centers[bucket_of]                                              # bucketCenterDelta (doubles)
        put(0, np.clip(np.floor(d * sf + 0.5) + scale_range, 0, scale_range * 2 + 1).astype(np.uint16))   # Math.round
        put(6, to_half_three(np.asarray(scales)[order]))
        put(12, to_half_three(q[order]))
    col = [40, 20, 20][lvl]
    put(col, np.asarray(rgba, np.uint8).reshape(n, 4)[order])
    if ncomp:
        s = np.asarray(sh_rows, np.float64).reshape(n, ncomp)[order]
        if lvl == 0:
            put(col + 4, s.astype(np.float32))
        elif lvl == 1:
            put(col + 4, to_half_three(s))
        else:
            lo, hi = sh_range
            put(col + 4, np.clip(np.floor((np.clip(s, lo, hi) - lo) / (hi - lo) * 255), 0, 255).astype(np.uint8))
    rows = table.tobytes()
    header = bytearray(4096)
    header[0:2] = bytes([0, 1])
    struct.pack_into("<IIII", header, 4, 1, 1, n, n)
    struct.pack_into("<H", header, 20, lvl)
    struct.pack_into("<fffff", header, 24, *scene_center, sh_range[0], sh_range[1])
    sec = bytearray(1024)
    storage = len(rows) + len(buckets_meta)
    struct.pack_into("<IIII", sec, 0, n, n, bucket_size if lvl else 0, n_buckets if lvl else 0)
    struct.pack_into("<f", sec, 16, block_size if lvl else 0.0)
    struct.pack_into("<H", sec, 20, 12 if lvl else 0)
    struct.pack_into("<IIII", sec, 24, scale_range if lvl else 0, storage, full if lvl else 0, len(partial_lengths) if lvl else 0)
    struct.pack_into("<H", sec, 40, sh_degree)
    return bytes(header) + bytes(sec) + buckets_meta + bytes(rows), order
