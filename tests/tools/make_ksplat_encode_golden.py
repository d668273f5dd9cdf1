"""tests/tools/make_ksplat_encode_golden.py — records tests/golden/ksplat_encode_ref.npz: seeded one-section level-0 .ksplat
images (gaussiansplats3d_amd.assets.write_ksplat(..., compression_level=0), patched with the edge rows below) and the bytes
the REFERENCE's own writer, SplatBuffer.generateFromUncompressedSplatArrays, returns for their rows.  Runs only where the
reference tree and Node exist: tests/tools/ksplat_encode_ref.mjs imports the reference's modules in place through
tests/tools/formats_loader.mjs.

The npz holds every input once (<input>_file), the manifest ({cases: [{name, input, compressionLevel, minimumAlpha, blockSize,
bucketSize, sceneCenter}]}) and per case the returned bytes (<name>_ksplat).  Inputs (300 to 640 splats; see the builders):
  sh0 / sh1 / sh2   a Gaussian cloud at SH degree 0 / 1 / 2, encoded at levels 0, 1, 2 with bucket_size 64 and block_size 4
                    (the central cells hold a few multiples of 64); sh0 also with bucket_size 4 and block_size 2.5
  exact             block_size 1, bucket_size 8: one cell holds exactly 8 splats (no open bucket is left of it), one holds 20
                    (fills, closes, reopens twice, leaves 4), the rest are spread over other cells
  lattice           integer-lattice centres, block_size 1: a centre on the far y face has yBlock == yBlocks and shares its id with
                    cell (x + 1, 0, z); the bucket's centre comes from whichever opened it, and the others' deltas hit both clamps
  flat              every centre has the same y: dims.y == 0, yBlocks == 0
  single            one splat survives minimum_alpha
  dropped           minimum_alpha 100 drops every third splat; the dropped rows hold the extreme SH values
  prefix            SH degree 1: a value of exactly 0 (and a -0, and a NaN) before the first negative one; a NaN scale, a -0 scale,
                    an all-zero quaternion
  nonneg / nonpos   SH degree 1 without a strictly negative (positive) value, with zeroes and NaNs: the whole scan is the
                    sequential prefix of the range rule, and its last zero leaves a bound that is no extreme of the values
  zero_sh           SH degree 2, every coefficient 0: the range falls back to -1.5 .. 1.5
  ties              centre deltas that are exact halves of the 16-bit step, both signs: Math.round sends them up
usage: python tests/tools/make_ksplat_encode_golden.py [<reference/src>]"""
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
NCOMP = {0: 0, 1: 9, 2: 24}


def level0(c, degree, seed, alpha=None, sh=None):
    """A level-0 image of centres c: seeded scales, rotations, colours and (unless given) SH."""
    rng = np.random.default_rng(seed)
    n = c.shape[0]
    scales = np.exp(rng.normal(-3.0, 0.7, size=(n, 3))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    rgba = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
    rgba[:, 3] = rng.integers(1, 256, size=n) if alpha is None else alpha
    if sh is None and degree:
        sh = rng.normal(0.0, 0.45, size=(n, NCOMP[degree]))
    data, _ = assets.write_ksplat(np.asarray(c, np.float32), scales, q, rgba, None if sh is None else np.asarray(sh, np.float32), degree, 0)
    return bytearray(data)


def patch(data, degree, row, column, values):
    """Overwrite floats of a level-0 row: column = float index in the row (0..2 centre, 3..5 scale, 6..9 rotation, 11.. SH)."""
    at = 5120 + (44 + 4 * NCOMP[degree]) * row + 4 * column
    raw = np.asarray(values, np.float32).tobytes()
    data[at:at + len(raw)] = raw


def inputs():
    out = {}
    rng = np.random.default_rng(7001)
    out["sh0"] = (level0(rng.normal(0.0, 1.6, size=(640, 3)) + [3.0, -2.0, 1.0], 0, 7002), 0)
    out["sh1"] = (level0(rng.normal(0.0, 1.6, size=(400, 3)), 1, 7003), 1)
    out["sh2"] = (level0(rng.normal(0.0, 1.6, size=(300, 3)), 2, 7004), 2)
    # exact: cell (0, 0, 0) 8 splats, cell (1, 0, 0) 20 splats, interleaved in file order; the corners pin min and max
    n = 300
    c = np.empty((n, 3))
    c[0], c[1] = (0.0, 0.0, 0.0), (12.0, 3.0, 3.0)
    cell = np.r_[np.zeros(7), np.ones(20)]
    rng.shuffle(cell)
    c[2:29] = np.c_[cell, np.zeros(27), np.zeros(27)] + rng.uniform(0.05, 0.95, size=(27, 3))
    c[29:] = np.c_[rng.integers(2, 12, n - 29), rng.integers(0, 3, n - 29), rng.integers(0, 3, n - 29)] + rng.uniform(0.05, 0.95, size=(n - 29, 3))
    out["exact"] = (level0(c, 0, 7005), 0)
    out["lattice"] = (level0(rng.integers(0, 5, size=(320, 3)).astype(np.float64), 0, 7006), 0)
    c = rng.normal(0.0, 2.0, size=(300, 3))
    c[:, 1] = 0.75
    out["flat"] = (level0(c, 1, 7007), 1)
    alpha = np.zeros(300, np.int64)
    alpha[137] = 200
    out["single"] = (level0(rng.normal(0.0, 2.0, size=(300, 3)), 1, 7008, alpha=alpha), 1)
    alpha = rng.integers(100, 256, size=360)
    alpha[::3] = rng.integers(0, 100, size=120)
    sh = rng.normal(0.0, 0.4, size=(360, 9))
    sh[::3] *= 4.0
    sh[3, 2], sh[6, 5] = -7.5, 8.25
    out["dropped"] = (level0(rng.normal(0.0, 2.0, size=(360, 3)), 1, 7009, alpha=alpha, sh=sh), 1)
    sh = rng.normal(0.0, 0.45, size=(300, 9))
    sh[0] = [0.5, 0.0, 0.25, -0.0, np.nan, 0.125, 0.0, 0.75, 0.3]
    sh[1, :4] = [0.0, np.nan, -0.4, 0.2]
    sh[40, 3], sh[41, 8] = np.nan, -0.0
    d = level0(rng.normal(0.0, 2.0, size=(300, 3)), 1, 7010, sh=sh)
    patch(d, 1, 5, 3, [np.nan, 0.02, -0.0])
    patch(d, 1, 9, 6, [0.0, 0.0, 0.0, 0.0])
    patch(d, 1, 11, 6, [0.0, -0.0, 0.0, -0.0])
    out["prefix"] = (d, 1)
    for name, sign, seed in (("nonneg", 1.0, 7011), ("nonpos", -1.0, 7012)):
        sh = sign * np.abs(rng.normal(0.0, 0.45, size=(300, 9)))
        sh[rng.random((300, 9)) < 0.1] = 0.0
        sh[2, 1], sh[17, 0], sh[299, 6:] = np.nan, np.nan, [0.0, sign * 0.015625, sign * 0.5]
        out[name] = (level0(rng.normal(0.0, 2.0, size=(300, 3)), 1, seed, sh=sh), 1)
    # ties: block_size 32767 / 2048 makes the centres' scale factor exactly 4096 and the first block's centre 32767 / 4096, so a
    # centre (2 * 32767 + k) / 8192 with k odd has delta * factor = k / 2: a tie Math.round sends up and rint sends to the even side
    c = rng.uniform(0.0, 15.5, size=(300, 3))
    c[0] = 0.0
    c[1:5] = (2 * 32767 + np.array([[5, 1, -3], [9, -7, 13], [-1, 3, 21], [-5, 5, -9]])) / 8192.0
    out["ties"] = (level0(c, 0, 7014), 0)
    out["zero_sh"] = (level0(rng.normal(0.0, 2.0, size=(300, 3)), 2, 7013, sh=np.zeros((300, 24))), 2)
    return out


def cases():
    out = []

    def add(name, inp, level, alpha=1, block=5.0, bucket=256, centre=(0.0, 0.0, 0.0)):
        out.append({"name": name, "input": inp, "compressionLevel": level, "minimumAlpha": alpha, "blockSize": block, "bucketSize": bucket,
                    "sceneCenter": list(centre)})

    for degree in (0, 1, 2):
        for level in (0, 1, 2):
            add(f"sh{degree}_l{level}", f"sh{degree}", level, block=4.0, bucket=64, centre=(0.5, -1.25, 2.0) if degree == 1 else (0.0, 0.0, 0.0))
    add("sh0_bucket4", "sh0", 1, block=2.5, bucket=4)
    add("sh0_defaults", "sh0", 1)
    for level in (0, 1):
        add(f"exact_l{level}", "exact", level, block=1.0, bucket=8)
        add(f"lattice_l{level}", "lattice", level, block=1.0, bucket=4)
    add("flat_l1", "flat", 1, block=1.5, bucket=16)
    add("single_l1", "single", 1)
    add("single_l2", "single", 2)
    add("dropped_l2", "dropped", 2, alpha=100, block=2.0, bucket=16)
    for level in (0, 1, 2):
        add(f"prefix_l{level}", "prefix", level, block=2.0, bucket=16)
    add("nonneg_l2", "nonneg", 2, block=3.0, bucket=32)
    add("nonpos_l2", "nonpos", 2, block=3.0, bucket=32)
    add("zero_sh_l2", "zero_sh", 2)
    add("ties_l1", "ties", 1, block=32767.0 / 2048.0, bucket=64)
    return out


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    assert os.path.isdir(ref_src), "reference not present"
    ins, cs = inputs(), cases()
    out = {name + "_file": np.frombuffer(bytes(data), np.uint8) for name, (data, _) in ins.items()}
    with tempfile.TemporaryDirectory() as d:
        for name, (data, _) in ins.items():
            open(os.path.join(d, name + ".ksplat"), "wb").write(bytes(data))
        json.dump([dict(c, file=c["input"] + ".ksplat") for c in cs], open(os.path.join(d, "cases.json"), "w"))
        subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "tests", "tools", "formats_loader.mjs"),
                               os.path.join(ROOT, "tests", "tools", "ksplat_encode_ref.mjs"), ref_src, d], cwd=os.path.join(ROOT, "oracle"))
        for c in cs:
            out[c["name"] + "_ksplat"] = np.fromfile(os.path.join(d, c["name"] + ".ksplat"), np.uint8)
    # what the cases are there to show, checked on the reference's own output
    u16 = lambda name: np.frombuffer(out[name + "_ksplat"].tobytes(), "<u2")      # noqa: E731
    sec = lambda name: np.frombuffer(out[name + "_ksplat"][4096:4096 + 44].tobytes(), "<u4")      # noqa: E731
    assert sec("single_l1")[0] == 1 and sec("dropped_l2")[0] == 240
    s = sec("lattice_l1")
    rows = out["lattice_l1_ksplat"][5120 + 4 * s[9] + 12 * s[3]:].reshape(-1, 24)
    centre = np.frombuffer(rows[:, :6].tobytes(), "<u2")
    assert (centre == 0).any() and (centre == 65535).any(), "the lattice case must hit both clamps"
    assert sec("exact_l1")[8] >= 3 and u16("exact_l1").size
    assert np.frombuffer(out["zero_sh_l2_ksplat"][36:44].tobytes(), "<f4").tolist() == [-1.5, 1.5]
    out["manifest"] = np.frombuffer(json.dumps({"cases": cs}).encode(), np.uint8)
    path = os.path.join(GOLDEN, "ksplat_encode_ref.npz")
    np.savez_compressed(path, **out)
    print(len(cs), "cases", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
