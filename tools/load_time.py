"""Load time of a scene file, file bytes -> a synchronised device, both paths in one process:
    python tools/load_time.py [--n 5800000] [--file NAME] [--format ksplat|ply|splat|compressed-ply|spz|inria-v2] [--sh-degree 0..3]
                              [--repeats 5] [--transform identity | 16 numbers] [--stream] [--out profiles/<tag>_load_time.txt]
  host    gs_asset_fill -> gs_mesh_upload (+ gs_mesh_upload_sh_u8) -> util.integer_centers -> gs_sorter_upload_centers
  device  gs_mesh_upload_asset + gs_sorter_upload_asset_centers (the per-splat decode on the card, csrc/asset_decode.hip)
  --stream adds the streamed reader (gs_asset_open_stream): the file is fed in 256 KiB appends (Constants.ProgressiveLoadSectionSize)
  and the rows that became ready are uploaded to a fresh mesh and sorter
    stream/1   after every append          stream/16  after every 16th append (and the last)
  timed from the first append to a synchronised device: the appends' copies and header work, every upload's staging, decode and
  Morton run.  The bytes are in memory, so this is the cost the loader adds to a download, not a download.  Printed beside the two
  whole-file paths, which it leaves as they are.
The file: $GS_DATA_DIR/<--file> when given (a name ending in .splat is one), else a seeded file of --n splats (the C3 count
by default) in --format, from the writers of gaussiansplats3d_amd.assets: a level-2 SH-2 .ksplat (the default), an INRIA-v1
PLY, a .splat, a PlayCanvas compressed PLY, a version-2 .spz or an INRIA-v2 codebook PLY with --sh-degree bands.  For .splat /
compressed PLY / .spz / INRIA-v2 PLY the asset keeps the file's rows and the host decodes them on its first fill, so both paths open a fresh asset inside the timed
region (for .spz that includes the inflate, on both paths).  --transform: the scene's static transform (Matrix4.elements, column-major; `identity` is what a static
Viewer passes for a scene without one), set on the asset so both paths bake it (gs_asset_set_transform).  Every repeat loads into a fresh mesh and sorter (a re-upload would skip the Morton sort); the two paths
alternate.  Prints median and spread (max - min) of both and the bytes each sends over PCIe; the device path passes when its
median is below the host path's by more than the larger spread."""
import argparse
import gzip
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiansplats3d_amd import Context, SplatMesh, assets, create_sort_worker, util
from gaussiansplats3d_amd import _lib as L


STREAM_APPEND = 262_144                                    # Constants.ProgressiveLoadSectionSize


def seeded_file(n):
    rng = np.random.default_rng(20260921)
    centers = rng.normal(size=(n, 3)) * 4.0
    scales = np.exp(rng.normal(-3.6, 0.5, size=(n, 3)))
    rot = rng.normal(size=(n, 4))
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    sh = rng.normal(0.0, 0.4, size=(n, 24)).astype(np.float32)
    return assets.write_ksplat(centers, scales, rot, rgba, sh, 2, 2, block_size=5.0, bucket_size=256)[0]


def seeded(fmt, n, sh_degree):
    """(bytes, SplatAsset fmt, description) of the seeded file in --format."""
    if fmt == "ksplat":
        return seeded_file(n), "ksplat", f"seeded level-2 SH-2 .ksplat, {n} splats"
    rng = np.random.default_rng(20260921)
    centers = rng.normal(size=(n, 3)) * 4.0
    log_scales = rng.normal(-3.6, 0.5, size=(n, 3))
    rot = rng.normal(size=(n, 4))
    ncoef = {0: 0, 1: 9, 2: 24, 3: 45}[sh_degree]
    if fmt == "splat":
        return assets.write_splat(centers, np.exp(log_scales), rot, rng.integers(0, 256, size=(n, 4), dtype=np.uint8)), "splat", \
            f"seeded .splat, {n} splats"
    sh = rng.normal(0.0, 0.4, size=(n, ncoef)).astype(np.float32) if ncoef else None
    if fmt == "spz":
        return assets.write_spz(centers, log_scales, rot, rng.random((n, 4)), sh), "spz", \
            f"seeded version-2 .spz, file SH degree {sh_degree}, {n} splats"
    if fmt == "compressed-ply":
        return assets.write_compressed_ply(centers, log_scales, rot, rng.random((n, 4)), sh), "ply", \
            f"seeded PlayCanvas compressed PLY, {ncoef} SH properties, {n} splats"
    if fmt == "inria-v2":
        return assets.write_inria_v2_ply(centers, log_scales, rot, rng.normal(size=(n, 3)), rng.normal(size=n), sh), "ply", \
            f"seeded INRIA-v2 codebook PLY, {ncoef} f_rest fields, {n} splats"
    return assets.write_ply(centers, log_scales, rot, rng.normal(size=(n, 3)), rng.normal(size=n), sh), "ply", \
        f"seeded INRIA-v1 PLY, {ncoef} f_rest properties, {n} splats"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", default="ksplat", choices=["ksplat", "ply", "splat", "compressed-ply", "spz", "inria-v2"])
    ap.add_argument("--sh-degree", type=int, default=2, choices=[0, 1, 2, 3], help="bands of a seeded ply / compressed-ply / spz / inria-v2")
    ap.add_argument("--n", type=int, default=5_800_000)
    ap.add_argument("--file", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--transform", nargs="+", default=None, metavar="M", help="`identity` or the 16 elements, column-major")
    ap.add_argument("--stream", action="store_true", help="also time the streamed reader: 256 KiB appends, uploads after every append and every 16th")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    transform = None
    if args.transform is not None:
        transform = np.eye(4).reshape(16) if args.transform == ["identity"] else np.array([float(v) for v in args.transform])
        if transform.size != 16:
            ap.error("--transform takes `identity` or 16 numbers")
    if args.file:
        path = os.path.join(os.environ.get("GS_DATA_DIR", "."), args.file)
        data, source = open(path, "rb").read(), args.file
        fmt = "splat" if args.file.lower().endswith(".splat") else ("spz" if args.file.lower().endswith(".spz") else None)
    else:
        data, fmt, source = seeded(args.format, args.n, args.sh_degree)

    def opened():
        a = assets.SplatAsset(data, fmt, 2)
        a.set_transform(transform)
        return a

    asset = opened()
    info = asset.info
    header = data[:data.index(b"end_header\n") + 11] if data[:3] == b"ply" else b""
    compressed = b"element chunk" in header
    inria_v2 = not compressed and b"element codebook_centers" in header
    spz = fmt == "spz" or data[:2] == b"\x1f\x8b"
    file_rows = fmt == "splat" or compressed or spz or inria_v2       # the asset keeps the file's rows
    n, deg, sh8 = info.splat_count, info.sh_degree, info.sh_level == 2 and info.sh_degree > 0
    ncoef = {0: 0, 1: 9, 2: 24}[deg]
    ctx = Context(0)

    def fresh():
        return SplatMesh(ctx, n, deg, spherical_harmonics_8bit=sh8), create_sort_worker(ctx, n)

    def host(mesh, worker):
        a = opened() if file_rows else asset
        f = a.fill(1, False)
        p = lambda a: a.ctypes.data if a is not None else None      # noqa: E731
        L.check(mesh.lib.gs_mesh_upload(mesh.handle, 0, n, p(f["centers"]), p(f["cov"]), None, p(f["rgba"]), p(f["sh_f16"])))
        if f["sh_u8"] is not None:
            L.check(mesh.lib.gs_mesh_upload_sh_u8(mesh.handle, 0, n, p(f["sh_u8"])))
        ci = util.integer_centers(f["centers"])
        L.check(worker.lib.gs_sorter_upload_centers(worker.handle, 0, n, ci.ctypes.data, None))
        if file_rows:
            a.close()

    def device(mesh, worker):
        a = opened() if file_rows else asset
        a.upload_to(mesh)
        a.upload_centers_to(worker)
        if file_rows:
            a.close()

    stream_fmt = fmt or ("ply" if data[:3] == b"ply" else "ksplat")
    uploads = {}

    def streamed(every):
        def path(mesh, worker):
            a = assets.SplatAssetStream(stream_fmt, 2, len(data))
            a.set_transform(transform)
            done = calls = 0
            ends = list(range(STREAM_APPEND, len(data), STREAM_APPEND)) + [len(data)]
            at = 0
            for k, end in enumerate(ends):
                ready = a.append(data[at:end], end == len(data)).splats_ready
                at = end
                if ready > done and ((k + 1) % every == 0 or end == len(data)):
                    a.upload_to(mesh, done, done, ready - done)
                    a.upload_centers_to(worker, done, done, ready - done)
                    done, calls = ready, calls + 1
            assert done == n
            uploads[every] = (len(ends), calls)
            a.close()
        return path

    paths = [("host", host), ("device", device)] + ([("stream/1", streamed(1)), ("stream/16", streamed(16))] if args.stream else [])
    times = {name: [] for name, _ in paths}
    for _ in range(args.repeats):
        for name, path in paths:
            mesh, worker = fresh()
            ctx.synchronize()
            t0 = time.perf_counter()
            path(mesh, worker)
            ctx.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            worker.terminate()
            mesh.dispose()
    if fmt == "splat":
        device_bytes = 2 * len(data)                                  # the rows, once for the mesh and once for the sorter
    elif spz:                                     # the position plane twice, the other planes once; the SH plane whole when the mesh keeps a band
        version, _, file_degree = struct.unpack_from("<IIB", gzip.decompress(data), 4)
        device_bytes = n * (2 * (9 if version == 2 else 6) + 10 + (3 * (0, 3, 8, 15)[file_degree] if ncoef else 0))
    elif compressed:                                                  # vertex rows + chunk rows twice, the SH bytes once
        sh_file = n * header.count(b"property uchar f_rest_")
        device_bytes = 2 * (len(data) - len(header) - sh_file) + (sh_file if ncoef else 0)
    elif inria_v2:                                                    # the index rows twice, the decoded codebook (20 pages of 256 floats) once
        device_bytes = 2 * n * (6 + header.count(b"property uchar ")) + 20 * 256 * 4
    elif data[:3] == b"ply":
        device_bytes = 2 * n * (44 + 4 * ncoef)                       # the level-0 image the host built from the PLY
    else:
        device_bytes = 2 * (len(data) - 4096 - 1024 * int(np.frombuffer(data[4:8], np.uint32)[0]))   # rows + bucket tables
    pcie = {"host": n * (12 + 24 + 4 + ncoef * (1 if sh8 else 2)) + n * 16, "device": device_bytes}
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float(max(v) - min(v)) for k, v in times.items()}
    lines = [f"load_time: {source}; file {len(data)} bytes, {n} splats, SH degree {deg}, compression level {info.compression_level}; "
             f"{args.repeats} repeats per path, alternating, fresh mesh + sorter each; scene transform "
             + ("none" if transform is None else " ".join(f"{v:g}" for v in transform))]
    for k in ("host", "device"):
        lines.append(f"{k:6s} median {med[k]:10.2f} ms  spread {spread[k]:8.2f} ms  PCIe {pcie[k]:12d} bytes ({pcie[k] / n:.1f} B/splat)  "
                     f"runs " + " ".join(f"{t:.2f}" for t in times[k]))
    for every in (1, 16) if args.stream else ():
        k = f"stream/{every}"
        lines.append(f"{k:9s} median {med[k]:10.2f} ms  spread {spread[k]:8.2f} ms  {uploads[every][0]} appends of {STREAM_APPEND} bytes, "
                     f"{uploads[every][1]} uploads  runs " + " ".join(f"{t:.2f}" for t in times[k]))
    gap, need = med["host"] - med["device"], max(spread["host"], spread["device"])
    lines.append(f"gap {gap:.2f} ms (x{med['host'] / med['device']:.1f}), larger spread {need:.2f} ms: " + ("PASS" if gap > need else "FAIL"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    asset.close()
    ctx.close()
    return 0 if gap > need else 1


if __name__ == "__main__":
    sys.exit(main())
