"""What tests/test_assets_inria_v2_ref.py (CPU) and tests/test_gpu_asset_inria_v2.py (-m gpu) share: the golden recorded by
tests/tools/make_inria_v2_golden.py (seeded INRIA-v2 codebook PLY files and what the reference's own INRIAV2PlyParser and SplatBuffer
fills return for them, in file order), loaded once and left unchanged."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def golden():
    """(arrays, manifest) of tests/golden/assets_inria_v2_ref.npz."""
    if not _CACHE:
        g = np.load(os.path.join(GOLDEN, "assets_inria_v2_ref.npz"))
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


def matrix():
    return golden()[0]["matrix"].copy()
