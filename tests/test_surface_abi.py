"""CPU tier: gs_mesh_surface is declared, exported and typed - and the ABI version did not move for it (the asset entry points
were added the same way)."""
import os
import re

import gaussiansplats3d_amd as g
from gaussiansplats3d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gs_mesh_surface_is_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+gs_mesh_surface\s*\(([^)]*)\)\s*;", code)
    assert decl, "include/gsplat_hip.h does not declare gs_mesh_surface"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 10
    assert params[0].startswith("gs_mesh*") and params[5].startswith("float ") and params[6].startswith("uint32_t*")
    assert hasattr(g.load(), "gs_mesh_surface"), "declared but not exported"
    res, args = _lib.SYMBOLS["gs_mesh_surface"]
    assert res is _lib.C.c_int and len(args) == 10 and args[5] is _lib.C.c_float


def test_the_abi_version_stays_5():
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", header).group(1)) == 5
    assert g.load().gs_abi_version() == 5


def test_the_python_mirror_offers_the_pass():
    from gaussiansplats3d_amd import SplatMesh, camera
    assert callable(SplatMesh.surface) and callable(camera.unproject)
