"""CPU tier: the device asset decode's two entry points (gs_mesh_upload_asset, gs_sorter_upload_asset_centers) are declared in
include/gsplat_hip.h, exported by the built library and typed in the ctypes table with the header's signatures; the ABI
version stays 5 (additive entry points, like the distance pass)."""
import ctypes as C
import os
import re

import gaussiansplats3d_amd as g
from gaussiansplats3d_amd import _lib, assets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"uint32_t": C.c_uint32, "int": C.c_int}


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/gsplat_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(C.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]])
    return C_TYPES[m.group(1)], args


def test_both_entry_points_are_declared_exported_and_typed():
    lib = g.load()
    for name, n_args in (("gs_mesh_upload_asset", 6), ("gs_sorter_upload_asset_centers", 6)):
        res, args = _declaration(name)
        assert len(args) == n_args
        assert hasattr(lib, name), f"{name} is not exported by libgsplat_hip.so"
        assert name in _lib.SYMBOLS, f"{name} is missing from the ctypes table"
        assert _lib.SYMBOLS[name] == (res, args), f"{name}: the ctypes table and the header disagree"
    assert lib.gs_abi_version() == 5


def test_header_names_the_reference_lines_they_replace():
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gs_mesh_upload_asset", "gs_sorter_upload_asset_centers"):
        at = text.index(f"int {name}(")
        comment = text[text.rindex("/*", 0, at):at]
        assert "Replaces" in comment and ".js:" in comment, name


def test_python_mirror_has_the_two_methods():
    assert callable(assets.SplatAsset.upload_to) and callable(assets.SplatAsset.upload_centers_to)
