"""CPU tier: gs_mesh_reorder is declared in include/gsplat_hip.h with the signature `int (gs_mesh*, uint32_t, uint32_t)`, exported
by the built library and typed in the ctypes table with the header's signature; the ABI version stays 5 (an additive entry point,
like gs_mesh_remove).  The plan's debug entry is exported and is not part of the public header."""
import ctypes as C
import os
import re

import gaussiansplats3d_amd as g
from gaussiansplats3d_amd import SplatMesh, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"uint32_t": C.c_uint32, "int": C.c_int}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat_hip.h")).read(), flags=re.S)


def test_the_entry_point_is_declared_exported_and_typed():
    m = re.search(r"\b(\w+)\s+gs_mesh_reorder\s*\(([^)]*)\)\s*;", _header())
    assert m, "gs_mesh_reorder is not declared in include/gsplat_hip.h"
    args = [a.strip() for a in m.group(2).split(",")]
    assert m.group(1) == "int" and args == ["gs_mesh* m", "uint32_t from", "uint32_t count"]
    typed = (C_TYPES[m.group(1)], [C.c_void_p if "*" in a else C_TYPES[a.split()[0]] for a in args])
    lib = g.load()
    assert hasattr(lib, "gs_mesh_reorder"), "gs_mesh_reorder is not exported by libgsplat_hip.so"
    assert _lib.SYMBOLS.get("gs_mesh_reorder") == typed, "the ctypes table and the header disagree"
    assert lib.gs_abi_version() == 5
    assert re.search(r"#define\s+GS_ABI_VERSION\s+5\b", _header())


def test_the_debug_entry_is_exported_and_not_public():
    assert hasattr(g.load(), "gs_debug_reorder_plan")
    assert "gs_debug_reorder_plan" not in _header()


def test_python_mirror_has_the_method():
    assert callable(SplatMesh.reorder)
