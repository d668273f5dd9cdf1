"""Convert a scene file (.ply: INRIA-v1, PlayCanvas compressed or INRIA-v2; .splat; .spz; a level-0 .ksplat) to a .ksplat on the
device: the reference's util/create-ksplat.js, with its arguments, through gs_asset_encode_ksplat.  The file is byte for byte what
SplatBuffer.generateFromUncompressedSplatArrays writes for the input's level-0 rows in file order - one section, no
SplatPartitioner.  Prints the time to open the input (read + parse), to encode it (upload of the file's rows, the kernels, the copy
back and the re-open of the result) and to write the output.

usage: python tools/create_ksplat.py IN OUT [compression level = 0] [alpha removal threshold = 1] [scene center = "0,0,0"]
                                     [block size = 5.0] [bucket size = 256] [spherical harmonics level = 0]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gaussiansplats3d_amd import Context, assets


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 1
    src, dst = argv[1], argv[2]
    level = int(argv[3]) if len(argv) > 3 else 0
    alpha = int(argv[4]) if len(argv) > 4 else 1
    centre = [float(v) for v in argv[5].split(",")] if len(argv) > 5 else [0.0, 0.0, 0.0]
    block = float(argv[6]) if len(argv) > 6 else 5.0
    bucket = int(argv[7]) if len(argv) > 7 else 256
    degree = int(argv[8]) if len(argv) > 8 else 0
    fmt = "splat" if src.lower().endswith(".splat") else ("spz" if src.lower().endswith(".spz") else None)
    ctx = Context(0)
    t0 = time.perf_counter()
    with open(src, "rb") as f:
        data = f.read()
    asset = assets.SplatAsset(data, fmt, degree)
    t1 = time.perf_counter()
    out, _ = asset.encode_ksplat(ctx, compression_level=level, minimum_alpha=alpha, block_size=block, bucket_size=bucket, scene_center=centre)
    t2 = time.perf_counter()
    image = out.to_bytes()
    with open(dst, "wb") as f:
        f.write(image)
    t3 = time.perf_counter()
    print(f"{src}: {asset.info.splat_count} splats, SH degree {asset.info.sh_degree}, {len(data) / 1e6:.1f} MB -> {dst}: level {level}, "
          f"{out.info.splat_count} splats, {len(image) / 1e6:.1f} MB")
    print(f"open {t1 - t0:.3f} s, encode {t2 - t1:.3f} s, write {t3 - t2:.3f} s")
    out.close()
    asset.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
