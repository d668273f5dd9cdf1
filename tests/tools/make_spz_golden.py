"""tests/tools/make_spz_golden.py — records tests/golden/assets_spz_ref.npz: seeded .spz files (the streams of
gaussiansplats3d_amd.assets.spz_stream, patched with the edge rows below, gzipped) and what the REFERENCE's own SpzLoader
and SplatBuffer fills return for them.  Runs only where the reference tree and Node exist: tests/tools/spz_ref.mjs imports
the reference's modules in place through tests/tools/formats_loader.mjs.

Files, 600 splats each (`reads` = the output degrees a file is read at, each executed on its own):
  v2_sh0 .. v2_sh3   version 2, fractionalBits 12, file SH degree 0 / 1 / 2 / 3, each read at 0, 1 and 2; alphas 0 / 39 / 40
  v2_fb0, _fb31, _fb40   version 2, SH 0, fractionalBits 0 (integer positions), 31 (1 << 31 is negative: every centre changes
                     sign and shrinks by 2^31) and 40 (the shift count is taken mod 32: reads as 8)
  v1_sh1             version 1: half positions, among them +-0, subnormals, +-inf and NaN
  exhaustive         version 2, SH 1, planes that run through every value instead of random ones: every scale, colour, alpha
                     and SH byte; positions -2^23, 2^23 - 1, 0 and -1; rotation bytes with x^2 + y^2 + z^2 below 1, above 1,
                     (255, 255, 255), (0, 0, 0) and the centre (127, 128, 127)
Everything but the SH of a file is the same at every output degree; the generator ASSERTS that on the reference's output
and stores those arrays once per file (<file>_centers ...), the SH per read (<file>_d<degree>_sh, _xf_sh).  The npz holds
the gzipped input files themselves, so the tests never depend on a zlib version.
usage: python tests/tools/make_spz_golden.py [<reference/src>]"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gaussiansplats3d_amd import assets  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLUSTER = np.array([2.4, 2.6, -2.5])
N = 600
DIM = {0: 0, 1: 3, 2: 8, 3: 15}
SHARED = ("centers", "cov32", "cov16", "rgba1", "rgba40", "scales", "rotations", "xf_centers", "xf_cov32", "xf_cov16")


def splats(degree, seed):
    rng = np.random.default_rng(seed)
    c = CLUSTER + rng.normal(0.0, 0.6, size=(N, 3))
    log_scales = rng.normal(-3.4, 0.6, size=(N, 3))
    q = rng.normal(size=(N, 4))
    rgba = rng.random((N, 4))
    sh = rng.normal(0.0, 0.4, size=(N, 3 * DIM[degree])) if degree else None
    return rng, c, log_scales, q, rgba, sh


def planes(stream, version, degree):
    """{plane: (offset, stride)} of an uncompressed stream."""
    out, at = {}, 16
    for name, stride in (("positions", 9 if version == 2 else 6), ("alphas", 1), ("colours", 3), ("scales", 3), ("rotations", 3),
                         ("sh", 3 * DIM[degree])):
        out[name] = (at, stride)
        at += stride * N
    assert at == len(stream)
    return out


def spz_files():
    out = []

    def add(name, stream, reads, visible=True):
        out.append({"name": name, "data": gzip.compress(bytes(stream), 6, mtime=0), "reads": reads, "visible": visible})

    for degree in range(4):
        rng, c, ls, q, rgba, sh = splats(degree, 301 + degree)
        stream = bytearray(assets.spz_stream(c, ls, q, rgba, sh, 2, 12))
        at = planes(stream, 2, degree)["alphas"][0]
        stream[at + 3], stream[at + 4], stream[at + 5] = 0, 39, 40
        add(f"v2_sh{degree}", stream, [0, 1, 2])
    for bits, visible in ((0, True), (31, False), (40, True)):
        rng, c, ls, q, rgba, _ = splats(0, 310 + bits)
        stream = bytearray(assets.spz_stream(c, ls, q, rgba, None, 2, bits % 32 if bits != 31 else 8))
        stream[13] = bits
        stream[planes(stream, 2, 0)["alphas"][0] + 7] = 20
        add(f"v2_fb{bits}", stream, [0], visible)
    rng, c, ls, q, rgba, sh = splats(1, 320)
    stream = bytearray(assets.spz_stream(c, ls, q, rgba, sh, 1))
    p = planes(stream, 1, 1)
    halves = np.frombuffer(bytes(stream[p["positions"][0]:p["positions"][0] + 6 * N]), "<u2").copy()
    special = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7C01, 0xFE00, 0x7FFF]
    halves[3 * 10:3 * 10 + len(special)] = special                    # splats 10 .. 14
    stream[p["positions"][0]:p["positions"][0] + 6 * N] = halves.astype("<u2").tobytes()
    stream[p["alphas"][0] + 3] = 12
    add("v1_sh1", stream, [1])
    # ---- the exhaustive file
    rng, c, ls, q, rgba, sh = splats(1, 330)
    stream = bytearray(assets.spz_stream(c, ls, q, rgba, sh, 2, 12))
    p = planes(stream, 2, 1)
    every = np.arange(N * 9) % 256
    stream[p["scales"][0]:p["scales"][0] + 3 * N] = (np.arange(3 * N) % 256).astype(np.uint8).tobytes()
    stream[p["colours"][0]:p["colours"][0] + 3 * N] = ((np.arange(3 * N) * 7 + 3) % 256).astype(np.uint8).tobytes()    # 7 is coprime to 256
    stream[p["alphas"][0]:p["alphas"][0] + N] = (np.arange(N) % 256).astype(np.uint8).tobytes()
    stream[p["sh"][0]:p["sh"][0] + 9 * N] = ((every * 5 + 1) % 256).astype(np.uint8).tobytes()
    for k, fixed in enumerate((0x800000, 0x7FFFFF, 0x000000, 0xFFFFFF)):                                   # splats 20 .. 23, every axis
        for axis in range(3):
            o = p["positions"][0] + 9 * (20 + k) + 3 * axis
            stream[o:o + 3] = int(fixed).to_bytes(3, "little")
    rot = [(255, 255, 255), (0, 0, 0), (127, 128, 127), (255, 0, 255), (255, 128, 128), (128, 128, 0), (200, 200, 100), (217, 128, 128),
           (218, 128, 128), (127, 127, 127), (128, 128, 128), (0, 255, 0)]
    for k, r in enumerate(rot):                                                                            # splats 30 ..
        o = p["rotations"][0] + 3 * (30 + k)
        stream[o:o + 3] = bytes(r)
    add("exhaustive", stream, [1])
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    assert os.path.isdir(ref_src), "reference not present"
    files = spz_files()
    matrix = np.load(os.path.join(GOLDEN, "assets_transform_ref_sh0.npz"))["nonuniform_matrix"]   # asset_transform_cases' nonuniform
    out, man = {"matrix": matrix}, {"cases": []}
    with tempfile.TemporaryDirectory() as d:
        matrix.astype("<f8").tofile(os.path.join(d, "matrix.f64"))
        runs = []
        for f in files:
            open(os.path.join(d, f["name"] + ".spz"), "wb").write(f["data"])
            out[f["name"] + "_file"] = np.frombuffer(f["data"], np.uint8)
            for deg in f["reads"]:
                runs.append({"name": f"{f['name']}_d{deg}", "file": f["name"] + ".spz", "degree": deg})
                man["cases"].append({"name": f"{f['name']}_d{deg}", "base": f["name"], "file": f["name"] + "_file", "fmt": "spz", "degree": deg,
                                     "visible": f["visible"]})
        json.dump(runs, open(os.path.join(d, "cases.json"), "w"))
        subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "tests", "tools", "formats_loader.mjs"),
                               os.path.join(ROOT, "tests", "tools", "spz_ref.mjs"), ref_src, d], cwd=os.path.join(ROOT, "oracle"))
        ref = json.load(open(os.path.join(d, "manifest.json")))
        header = {f["name"]: gzip.decompress(f["data"])[:16] for f in files}
        for entry in man["cases"]:
            name, base, r = entry["name"], entry["base"], ref[entry["name"]]
            n, nc = r["splatCount"], r["ncoef"]
            assert n == N and r["shDegree"] == min(entry["degree"], header[base][12], 2) and r["compressionLevel"] == 0 and r["shLevel"] == 1, (name, r)
            entry.update(splatCount=n, shDegree=r["shDegree"], ncoef=nc)
            rd = lambda ext, dt, w: np.fromfile(os.path.join(d, f"{name}_{ext}"), dt).reshape(n, w)      # noqa: E731
            got = {"centers": rd("centers.f32", np.float32, 3), "cov32": rd("cov.f32", np.float32, 6), "cov16": rd("cov.u16", np.uint16, 6),
                   "rgba1": rd("rgba1.u8", np.uint8, 4), "rgba40": rd("rgba40.u8", np.uint8, 4), "scales": rd("scales.f32", np.float32, 3),
                   "rotations": rd("rotations.f32", np.float32, 4), "xf_centers": rd("xf_centers.f32", np.float32, 3),
                   "xf_cov32": rd("xf_cov.f32", np.float32, 6), "xf_cov16": rd("xf_cov.u16", np.uint16, 6)}
            for k in SHARED:
                if f"{base}_{k}" in out:              # the same at every output degree, bit for bit (NaNs included: one process wrote both)
                    assert np.array_equal(out[f"{base}_{k}"].view(np.uint8), got[k].view(np.uint8)), (name, k)
                else:
                    out[f"{base}_{k}"] = got[k]
            if nc:
                out[f"{name}_sh"], out[f"{name}_xf_sh"] = rd("sh.u16", np.uint16, nc), rd("xf_sh.u16", np.uint16, nc)
            nan = np.isnan(got["centers"]).any(axis=1) | np.isnan(got["cov32"]).any(axis=1) | np.isnan(got["rotations"]).any(axis=1)
            entry["splatsWithNaN"] = int(nan.sum())
            assert nan.mean() < 0.05, (name, int(nan.sum()))
    out["manifest"] = np.frombuffer(json.dumps(man).encode(), np.uint8)
    path = os.path.join(GOLDEN, "assets_spz_ref.npz")
    np.savez_compressed(path, **out)
    print({e["name"]: e["splatsWithNaN"] for e in man["cases"]}, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
