"""CPU tier: the two capacity calls (gs_mesh_resize, gs_sorter_resize) are declared in include/gsplat_hip.h with the signature
`int f(object*, uint32_t max_splat_count)`, exported by the built library and typed alike in the ctypes table; the ABI version
stays 5 (additive entry points); the Python mirrors and the worker's `resize` message exist."""
import ctypes as C
import os
import re

import gaussiansplats3d_amd as g
from gaussiansplats3d_amd import SortWorker, SplatMesh, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {"gs_mesh_resize": "gs_mesh* m, uint32_t max_splat_count", "gs_sorter_resize": "gs_sorter* s, uint32_t max_splat_count"}


def header():
    return open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()


def test_both_calls_are_declared_with_the_signature():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, args in SIGNATURES.items():
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in include/gsplat_hip.h"
        assert m.group(1) == "int" and " ".join(m.group(2).split()) == args, name


def test_both_calls_are_exported_and_typed_alike():
    lib = g.load()
    for name in SIGNATURES:
        assert hasattr(lib, name), f"{name} is not exported by libgsplat_hip.so"
        assert name in _lib.SYMBOLS, f"{name} is missing from the ctypes table"
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_uint32]), name
    assert _lib.SYMBOLS["gs_mesh_resize"] == _lib.SYMBOLS["gs_sorter_resize"]


def test_the_abi_version_stays_5():
    assert g.load().gs_abi_version() == 5
    assert re.search(r"#define\s+GS_ABI_VERSION\s+5\b", header())


def test_the_header_says_what_a_refusal_and_the_same_capacity_do():
    text = header()
    for name in SIGNATURES:
        at = text.index(f"int {name}(")
        comment = text[text.rindex("/*", 0, at):at]
        assert "GS_ERR_INVALID" in comment and "GS_ERR_NOMEM" in comment and "nothing happens" in comment, name
        assert "Viewer.js:" in comment, name


def test_python_mirrors_exist():
    assert callable(SplatMesh.resize) and callable(SortWorker.resize)
