"""tests/tools/make_formats_golden.py — records tests/golden/assets_formats_ref.npz: seeded .splat and PlayCanvas compressed
PLY files (written with gaussiansplats3d_amd.assets.write_splat / write_compressed_ply, then patched with the edge rows
below) and what the REFERENCE's own parsers and SplatBuffer fills return for them.  Runs only where the reference tree and
Node exist: tests/tools/formats_ref.mjs imports the reference's modules in place through tests/tools/formats_loader.mjs.

Cases (formats_cases() below; `reads` = the output degrees the file is read at, each its own recorded result):
  splat        500 rows; rotation bytes 0 / 255 / all-128 (length 0), alpha 0 / 39 / 40
  pc_sh0       600 splats (chunks of 256 + 256 + 88), no `sh` element, no colour extremes: the progressive path (the
               whole-file path throws on such a file)
  pc_sh0_ext   ... with min_r .. max_b; colour lerps that land on .5
  pc_sh1       9 SH properties, a `comment` line, the chunk properties in another order, colour extremes
  pc_sh2       24 SH properties, read at degree 2 and at 0
  pc_sh3       45 SH properties, read at degree 2 and at 1
Most rotation words are packed unit quaternions; a dozen per case are random words and four are 0x3FFFFFFF under each of
the top two bits (sqrt of a negative: NaN).
The generator asserts that fewer than 5 % of the splats of each case carry a NaN.
usage: python tests/tools/make_formats_golden.py [<reference/src>]"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gaussiansplats3d_amd import assets  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLUSTER = np.array([2.4, 2.6, -2.5])


def splats(n, ncoef, seed):
    rng = np.random.default_rng(seed)
    c = CLUSTER + rng.normal(0.0, 0.6, size=(n, 3))
    log_scales = rng.normal(-3.4, 0.6, size=(n, 3))
    q = rng.normal(size=(n, 4))
    rgba = rng.random((n, 4))
    sh = rng.normal(0.0, 0.5, size=(n, ncoef)) if ncoef else None
    return rng, c, log_scales, q, rgba, sh


def patch_chunk(data, chunk, name, value):
    """Overwrites float property `name` of chunk row `chunk` in a compressed PLY."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    names = []
    for line in data[:end].decode().split("\n"):
        w = line.split(" ")
        if w[0] == "element" and w[1] != "chunk":
            break
        if w[0] == "property":
            names.append(w[2])
    struct.pack_into("<f", data, end + 4 * (len(names) * chunk + names.index(name)), value)


def vertex_base(data):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().split("\n")
    nchunk = next(int(l.split(" ")[2]) for l in head if l.startswith("element chunk"))
    nprop = 0
    for line in head:
        if line.startswith("element vertex"):
            break
        nprop += line.startswith("property")
    return end + 4 * nprop * nchunk


def formats_cases():
    out = []
    # ---- .splat
    rng, c, ls, q, rgba, _ = splats(500, 0, 101)
    data = bytearray(assets.write_splat(c, np.exp(ls), q, (rgba * 255).astype(np.uint8)))
    for row, rot in ((0, (0, 0, 0, 0)), (1, (255, 255, 255, 255)), (2, (128, 128, 128, 128)), (6, (0, 255, 128, 127))):
        data[32 * row + 28:32 * row + 32] = bytes(rot)
    for row, alpha in ((3, 0), (4, 39), (5, 40)):
        data[32 * row + 27] = alpha
    out.append({"name": "splat", "data": bytes(data), "kind": "splat", "fmt": "splat", "reads": [0]})
    # ---- compressed PLY
    order = ["max_scale_z", "min_x", "max_x", "min_y", "max_y", "min_z", "max_z", "min_r", "max_b", "min_scale_x", "max_scale_x",
             "min_g", "min_scale_y", "max_scale_y", "max_r", "min_scale_z", "max_g", "min_b"]
    spec = [("pc_sh0", 0, False, "progressive", [0], None, None), ("pc_sh0_ext", 0, True, "progressive", [0], None, None),
            ("pc_sh1", 9, True, "whole", [1], order, "written by make_formats_golden.py"),
            ("pc_sh2", 24, False, "whole", [2, 0], None, None), ("pc_sh3", 45, True, "whole", [2, 1], None, None)]
    for k, (name, ncoef, ext, kind, reads, chunk_order, comment) in enumerate(spec):
        n = 600
        rng, c, ls, q, rgba, sh = splats(n, ncoef, 202 + k)
        words = {int(i): int(w) for i, w in zip(rng.choice(n, 12, replace=False), rng.integers(0, 1 << 32, 12, dtype=np.uint64))}
        for top, i in enumerate(rng.choice(np.setdiff1d(np.arange(n), list(words)), 4, replace=False)):
            words[int(i)] = (top << 30) | 0x3FFFFFFF                 # a = b = c = sqrt(2) / 2: the missing component is sqrt(-0.5)
        data = bytearray(assets.write_compressed_ply(c, ls, q, rgba, sh, ext, chunk_order, comment, words))
        if ext:
            # chunk 1: red lerps to 127.5 at c = 1, green to -127.5 (Math.round(-127.5) = -127, clamped), blue to 0.5 at c = 0
            for nm, v in (("min_r", 0.0), ("max_r", 0.5), ("min_g", 0.0), ("max_g", -0.5), ("min_b", 0.5 / 255), ("max_b", 1.0)):
                patch_chunk(data, 1, nm, v)
            vb = vertex_base(data)
            for i in range(256, 256 + 40):
                old = struct.unpack_from("<I", data, vb + 16 * i + 12)[0]
                new = (0xFF << 24) | (0xFF << 16) | (0x00 << 8) | (old & 0xFF) if i % 2 == 0 else old
                struct.pack_into("<I", data, vb + 16 * i + 12, new)
        out.append({"name": name, "data": bytes(data), "kind": kind, "fmt": "ply", "reads": reads})
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    assert os.path.isdir(ref_src), "reference not present"
    cases = formats_cases()
    matrix = np.load(os.path.join(GOLDEN, "assets_transform_ref_sh0.npz"))["nonuniform_matrix"]   # asset_transform_cases' nonuniform
    out, man = {"matrix": matrix}, {"cases": []}
    with tempfile.TemporaryDirectory() as d:
        matrix.astype("<f8").tofile(os.path.join(d, "matrix.f64"))
        runs = []
        for c in cases:
            open(os.path.join(d, c["name"] + ".bin"), "wb").write(c["data"])
            out[c["name"] + "_file"] = np.frombuffer(c["data"], np.uint8)
            for deg in c["reads"]:
                runs.append({"name": f"{c['name']}_d{deg}", "file": c["name"] + ".bin", "kind": c["kind"], "degree": deg})
                man["cases"].append({"name": f"{c['name']}_d{deg}", "file": c["name"] + "_file", "fmt": c["fmt"], "degree": deg})
        json.dump(runs, open(os.path.join(d, "cases.json"), "w"))
        subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "tests", "tools", "formats_loader.mjs"),
                               os.path.join(ROOT, "tests", "tools", "formats_ref.mjs"), ref_src, d], cwd=os.path.join(ROOT, "oracle"))
        ref = json.load(open(os.path.join(d, "manifest.json")))
        for entry in man["cases"]:
            name, r = entry["name"], ref[entry["name"]]
            n, nc = r["splatCount"], r["ncoef"]
            assert r["shDegree"] == min(entry["degree"], 2) and r["compressionLevel"] == 0 and r["shLevel"] == 1, (name, r)
            entry.update(splatCount=n, shDegree=r["shDegree"], ncoef=nc)
            rd = lambda ext, dt, w: np.fromfile(os.path.join(d, f"{name}_{ext}"), dt).reshape(n, w)      # noqa: E731
            for tag in ("", "xf_"):
                out[f"{name}_{tag}centers"] = rd(f"{tag}centers.f32", np.float32, 3)
                out[f"{name}_{tag}cov32"] = rd(f"{tag}cov.f32", np.float32, 6)
                out[f"{name}_{tag}cov16"] = rd(f"{tag}cov.u16", np.uint16, 6)
                if nc and not tag:
                    out[f"{name}_sh"] = rd("sh.u16", np.uint16, nc)
            out[f"{name}_rgba1"], out[f"{name}_rgba40"] = rd("rgba1.u8", np.uint8, 4), rd("rgba40.u8", np.uint8, 4)
            out[f"{name}_scales"], out[f"{name}_rotations"] = rd("scales.f32", np.float32, 3), rd("rotations.f32", np.float32, 4)
            nan = np.isnan(out[f"{name}_centers"]).any(axis=1) | np.isnan(out[f"{name}_cov32"]).any(axis=1) | \
                np.isnan(out[f"{name}_rotations"]).any(axis=1) | np.isnan(out[f"{name}_xf_cov32"]).any(axis=1)
            entry["splatsWithNaN"] = int(nan.sum())
            assert nan.mean() < 0.05, (name, int(nan.sum()))
    out["manifest"] = np.frombuffer(json.dumps(man).encode(), np.uint8)
    path = os.path.join(GOLDEN, "assets_formats_ref.npz")
    np.savez_compressed(path, **out)
    print({e["name"]: e["splatsWithNaN"] for e in man["cases"]}, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
