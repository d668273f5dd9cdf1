"""tests/tools/make_assets_transform_golden.py — records tests/golden/assets_transform_ref_{sh0,sh1,sh2}.npz: what the
REFERENCE's own SplatBuffer fills return for the files of tests/golden/assets_ref_*.npz when they are handed a scene
transform, as SplatMesh.fillSplatDataArrays does in static mode (src/splatmesh/SplatMesh.js:1872-1899).  Runs only where
the reference tree and Node exist: tests/tools/assets_transform_ref.mjs imports src/loaders/SplatBuffer.js and
src/loaders/ply/INRIAV1PlyParser.js in place, with 'three' resolved to oracle/three_min.mjs (oracle/three_loader.mjs).

Inputs are NOT stored again: the PLY bytes and the gen0 / gen1 / gen2 .ksplat bytes stay in assets_ref_*.npz.  Per tag x
transform (identity, rigid, uniform, nonuniform, mirror; built with Matrix4.compose in the .mjs): centres fp32, covariances
fp32 and half bits, SH at max(1, level), and the 16 doubles of each matrix.
usage: python tests/tools/make_assets_transform_golden.py [<reference/src>]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = ["ply", "gen0", "gen1", "gen2"]


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    assert os.path.isdir(ref_src), "reference not present"
    for case in ("sh2", "sh1", "sh0"):
        g = np.load(os.path.join(GOLDEN, f"assets_ref_{case}.npz"))
        old = json.loads(bytes(g["manifest"]).decode())
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "in.ply"), "wb").write(bytes(g["ply_bytes"]))
            for level in (0, 1, 2):
                open(os.path.join(d, f"gen{level}.ksplat"), "wb").write(bytes(g[f"gen{level}_ksplat"]))
            subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                                   os.path.join(ROOT, "tests", "tools", "assets_transform_ref.mjs"), ref_src, d, str(old["shDegree"])],
                                  cwd=os.path.join(ROOT, "oracle"))
            man = json.load(open(os.path.join(d, "transform_manifest.json")))
            out = {"manifest": np.frombuffer(json.dumps(man).encode(), np.uint8)}
            for name in man["transforms"]:
                out[f"{name}_matrix"] = np.fromfile(os.path.join(d, f"{name}_matrix.f64"), np.float64)
            for tag in TAGS:
                b, ob = man["buffers"][tag], old["buffers"][tag]
                n, nc = b["splatCount"], b["ncoef"]
                assert (n, nc, b["shLevel"], b["compressionLevel"]) == (ob["splatCount"], ob["ncoef"], ob["shLevel"], ob["compressionLevel"])
                for name in man["transforms"]:
                    rd = lambda ext, dt: np.fromfile(os.path.join(d, f"{tag}_{name}_{ext}"), dt)      # noqa: E731
                    out[f"{tag}_{name}_centers"] = rd("centers.f32", np.float32).reshape(n, 3)
                    out[f"{tag}_{name}_cov32"] = rd("cov.f32", np.float32).reshape(n, 6)
                    out[f"{tag}_{name}_cov16"] = rd("cov.u16", np.uint16).reshape(n, 6)
                    st = b["stats"][name]
                    assert st["finite"] and not st["halfOverflow"], (case, tag, name, st)
                    if nc:
                        sh = (rd("sh.u8", np.uint8) if b["shLevel"] == 2 else rd("sh.u16", np.uint16)).reshape(n, nc)
                        out[f"{tag}_{name}_sh"] = sh
                        if name == "identity":
                            # the consistency check: the identity transform moves exactly as many SH values as the old golden's
                            # manifest says (1304 of 9960 for sh2 / gen2, 0 for levels 0 / 1 and the PLY)
                            changed = int((sh != g[f"{tag}_sh"]).sum())
                            assert changed == ob["shValuesChangedByIdentityTransform"] == st["shChanged"], (case, tag, changed)
        path = os.path.join(GOLDEN, f"assets_transform_ref_{case}.npz")
        np.savez_compressed(path, **out)
        print(case, {t: {k: (v["shChanged"], v["shOnRail"]) for k, v in man["buffers"][t]["stats"].items()} for t in TAGS},
              os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
