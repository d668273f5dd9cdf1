"""Multi-section .ksplat files for the tests: assets.write_ksplat writes one section, join() puts several into one file."""
import struct

import numpy as np

from gaussiansplats3d_amd import assets

HEADER, SECTION_HEADER = 4096, 1024
BUCKET_SIZE = 64


def join(files):
    """Single-section .ksplat files of ONE compression level -> one file with their sections in order.  The main header is the first
    file's (level, scene centre, 8-bit SH range) with the section and splat counts patched; then the 1024-byte section headers,
    then the sections' bodies (partial bucket lengths, bucket centres, rows)."""
    assert len({struct.unpack_from("<H", f, 20)[0] for f in files}) == 1, "the sections must share a compression level"
    assert all(struct.unpack_from("<I", f, 4)[0] == 1 for f in files)
    head = bytearray(files[0][:HEADER])
    total = sum(struct.unpack_from("<I", f, 12)[0] for f in files)
    struct.pack_into("<IIII", head, 4, len(files), len(files), total, total)
    return (bytes(head) + b"".join(f[HEADER:HEADER + SECTION_HEADER] for f in files)
            + b"".join(f[HEADER + SECTION_HEADER:] for f in files))


def section_headers(data):
    """Per section: splats, bucket size, buckets, full and partial buckets, SH degree, as the file says."""
    out = []
    for s in range(struct.unpack_from("<I", data, 4)[0]):
        h = HEADER + SECTION_HEADER * s
        out.append({"splats": struct.unpack_from("<I", data, h + 4)[0], "bucket_size": struct.unpack_from("<I", data, h + 8)[0],
                    "buckets": struct.unpack_from("<I", data, h + 12)[0], "full": struct.unpack_from("<I", data, h + 32)[0],
                    "partial": struct.unpack_from("<I", data, h + 36)[0], "sh_degree": struct.unpack_from("<H", data, h + 40)[0]})
    return out


def _section(n, sh_degree, level, seed):
    rng = np.random.default_rng(seed)
    # long in x, thin in y and z: a few 4-unit blocks hold most splats (full buckets of 64), the ends hold partial ones
    centers = rng.normal(size=(n, 3)) * np.array([2.5, 0.4, 0.4]) + np.array([0.0, 0.0, 0.3 * seed])
    scales = np.exp(rng.normal(-3.0, 0.5, size=(n, 3)))
    rot = rng.normal(size=(n, 4))
    rgba = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    ncomp = {0: 0, 1: 9, 2: 24}[sh_degree]
    sh = rng.normal(0.0, 0.4, size=(n, ncomp)) if ncomp else None
    return assets.write_ksplat(centers, scales, rot, rgba, sh, sh_degree, level, block_size=4.0, bucket_size=BUCKET_SIZE,
                               sh_range=(-1.2, 1.3))[0]


_FILES = {}


def three_sections(level, degrees):
    """301 splats of SH degree degrees[0], an EMPTY section of the same degree, 310 splats of degrees[1]: the file's degree is the
    smaller one, and the rows of the two sections have different sizes when the degrees differ."""
    key = (level, tuple(degrees))
    if key not in _FILES:
        _FILES[key] = join([_section(301, degrees[0], level, 1), _section(0, degrees[0], level, 2), _section(310, degrees[1], level, 3)])
    return _FILES[key]
