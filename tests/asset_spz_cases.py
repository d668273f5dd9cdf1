"""What tests/test_assets_spz_ref.py (CPU) and tests/test_gpu_asset_spz.py (-m gpu) share: the golden recorded by
tests/tools/make_spz_golden.py (seeded .spz files and what the reference's own SpzLoader and fills return for them), loaded
once and left unchanged.  Everything but the SH of a file is the same at every output degree (the generator asserts it on
the reference's output), so those arrays are stored once per file: array(name, key) finds either."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def golden():
    """(arrays, manifest) of tests/golden/assets_spz_ref.npz."""
    if not _CACHE:
        g = np.load(os.path.join(GOLDEN, "assets_spz_ref.npz"))
        _CACHE["g"] = {k: g[k] for k in g.files}
        _CACHE["man"] = json.loads(bytes(g["manifest"]).decode())
    return _CACHE["g"], _CACHE["man"]


def cases():
    return [c["name"] for c in golden()[1]["cases"]]


def case(name):
    """(file bytes, fmt, degree the file is read at, manifest entry)."""
    g, man = golden()
    entry = next(c for c in man["cases"] if c["name"] == name)
    return bytes(g[entry["file"]]), entry["fmt"], entry["degree"], entry


def array(name, key):
    """The recorded array `key` of read `name`: per read for the SH (sh, xf_sh), per file for the rest."""
    g, man = golden()
    entry = next(c for c in man["cases"] if c["name"] == name)
    return g[f"{name}_{key}"] if key in ("sh", "xf_sh") else g[f"{entry['base']}_{key}"]


def matrix():
    return golden()[0]["matrix"].copy()
