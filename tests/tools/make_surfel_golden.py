"""tests/tools/make_surfel_golden.py - records what the REFERENCE's own, unmodified SplatMaterial2D shader strings and blend state
compute on a real GLES 3 rasteriser (Mesa llvmpipe, headless through tests/tools/gl_surfel.c over oracle/gl_ref.c) for the cases
of tests/surfel_cases.py.  Runs only where the reference, Node and swrast_dri.so exist; the tests read the fixtures alone.

  tests/golden/surfel_gl_ref.npz    per vertex case the transform feedback of every splat whose gl_Position the shader wrote:
  tests/golden/surfel_gl_ref2.npz   `written_<case>` bool [n], `vs_<case>` float32 [m, 24] = gl_Position.xy of the 4 corners,
                                    gl_Position.z, vColor, vT, vQuadCenter; per frame case the RGBA8 frame (glReadPixels, row 0 =
                                    bottom) drawn with the material's state, and the same for the designed cases; a JSON manifest: GL version, sha-256 of the shader
                                    strings, the measured model-to-GL distances per field class, the model's fp32 and per-splat
                                    rounded composites against every GL frame.  (Two files: each within 1 MiB.)
A second run writes byte-identical files.
usage: python tests/tools/make_surfel_golden.py"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import surfel_cases  # noqa: E402
import surfel_ref  # noqa: E402

from oracle import make_golden_gl as MGG  # noqa: E402
from oracle import make_golden_raster as MGR  # noqa: E402

REF_SRC = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRATCH = os.path.join(ROOT, "oracle", "_ref", "surfel")


def _lib():
    os.makedirs(SCRATCH, exist_ok=True)
    so = os.path.join(SCRATCH, "libglsurfel.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-o", so, os.path.join(ROOT, "tests", "tools", "gl_surfel.c"),
                           "-ldl", "-lm"])
    lib = C.CDLL(so)
    v, r = C.create_string_buffer(256), C.create_string_buffer(256)
    rc = lib.glref_init(v, r, 256)
    assert rc == 0, f"glref_init: {rc}"
    return lib, v.value.decode(), r.value.decode()


BUILDS = {"base0": dict(maxSphericalHarmonicsDegree=0), "base2": dict(maxSphericalHarmonicsDegree=2),
          "effects0": dict(maxSphericalHarmonicsDegree=0, enableOptionalEffects=True),
          "dynamic2": dict(maxSphericalHarmonicsDegree=2, dynamicMode=True)}


def _shaders():
    json.dump([dict(name=k, **v) for k, v in BUILDS.items()], open(os.path.join(SCRATCH, "perms.json"), "w"))
    subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                           os.path.join(ROOT, "tests", "tools", "surfel_shader_dump.mjs"), REF_SRC, SCRATCH, os.path.join(SCRATCH, "perms.json")],
                          cwd=os.path.join(ROOT, "oracle"), stdout=subprocess.DEVNULL)
    out, shas = {}, {}
    for name in BUILDS:
        vert, frag = open(os.path.join(SCRATCH, name + ".vert")).read(), open(os.path.join(SCRATCH, name + ".frag")).read()
        shas[name] = dict(vert_sha256=hashlib.sha256(vert.encode()).hexdigest(), frag_sha256=hashlib.sha256(frag.encode()).hexdigest())
        out[name] = (vert.encode(), frag.encode())
    return out, shas


def harness_case(case):
    """A tests/surfel_cases.py case in the shape oracle/make_golden_raster.harness_inputs takes: the scale / rotation tuples in
    the covariance slot."""
    cam, n = case["camera"], case["centers"].shape[0]
    deg = case["sh_degree"]
    sh8 = case["sh8_range"] is not None
    if deg == 0:
        sampled = np.zeros((n, 0), np.float32)
    elif sh8:
        sampled = case["sh"].astype(np.float32) / np.float32(255.0)
    else:
        sampled = np.asarray(case["sh"], np.float16).astype(np.float32)
    build = "dynamic2" if case["transforms"] is not None else ("effects0" if case["opacity"] is not None else ("base2" if deg else "base0"))
    fade = case["fade"]
    u = dict(model_view=case["view"], projection=case["proj"], view_matrix=case["view_matrix"], camera_position=case["cam_pos"],
             focal=cam.focal(1.0 / float(case["inv_focal_adj"])), viewport=(case["width"], case["height"]),
             ortho_zoom=float(getattr(cam, "zoom", 1.0)), inverse_focal_adjustment=float(case["inv_focal_adj"]), splat_scale=1.0,
             orthographic=int(bool(getattr(cam, "is_orthographic", False))), point_cloud=0, sh_degree=deg,
             fade_in_complete=0 if fade else 1, scene_count=1 if case["scene_idx"] is None else int(case["scene_idx"].max()) + 1,
             scene_center=list(fade[0]) if fade else [0.0, 0.0, 0.0], fade_start_radius=fade[1] if fade else 0.0,
             transforms=case["transforms"] or [], scene_opacity=case["opacity"] or [], scene_visibility=case["visible"] or [],
             sh8_range=tuple(case["sh8_range"]) if sh8 else (-1.5, 1.5))
    return dict(build=build, centers=case["centers"], rgba=case["rgba"], cov=case["tuples"], cov_half=False, cov16=None, sh8=sh8,
                sh_stored=deg, sh_sampled=sampled, scene_idx=case["scene_idx"], uniforms=u)


def capture(lib, shaders, case):
    h = harness_case(case)
    sc, u, _keep = MGR.harness_inputs(h)
    vert, frag = shaders[h["build"]]
    out = np.zeros((sc.count, 4, 21), np.float32)
    rc = lib.glsurfel_capture_vertices(vert, frag, C.byref(sc), C.byref(u), C.c_uint32(sc.count), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, f"glsurfel_capture_vertices: {rc}"
    # the shader reached its end: w == 1 at every corner and not the base stage's rejection (0, 0, 2, 1)
    written = (out[:, :, 3] == 1.0).all(axis=1) & ~(out[:, :, 2] == 2.0).all(axis=1) & np.isfinite(out[:, :, 0:2]).all(axis=(1, 2))
    same = out[:, :1, 4:19]
    assert np.array_equal(np.broadcast_to(same, out[:, :, 4:19].shape)[written], out[:, :, 4:19][written]), "varyings differ between corners"
    packed = np.concatenate([out[:, :, 0:2].reshape(-1, 8), out[:, 0, 2:3], out[:, 0, 4:8], out[:, 0, 8:17], out[:, 0, 17:19]], axis=1)
    return written, np.ascontiguousarray(packed[written])


def draw(lib, shaders, case, order, dest):
    h = harness_case(case)
    sc, u, _keep = MGR.harness_inputs(h)
    vert, frag = shaders[h["build"]]
    w, hh = case["width"], case["height"]
    order = np.ascontiguousarray(order, np.uint32)
    depth = np.ascontiguousarray(dest["dest_depth"], np.float32) if dest else None
    dst = np.ascontiguousarray(dest["dest_rgba"], np.uint8) if dest else None
    out = np.zeros((hh, w, 4), np.uint8)
    rc = lib.glsurfel_draw_frame(vert, frag, C.byref(sc), C.byref(u), order.ctypes.data_as(C.c_void_p), C.c_uint32(order.shape[0]),
                                 C.c_int(w), C.c_int(hh), depth.ctypes.data_as(C.c_void_p) if depth is not None else None,
                                 C.c_int(1 if dest and dest["depth_unorm24"] else 0), dst.ctypes.data_as(C.c_void_p) if dst is not None else None,
                                 out.ctypes.data_as(C.c_void_p))
    assert rc == 0, f"glsurfel_draw_frame: {rc}"
    return out


def main():
    assert os.path.isdir(REF_SRC), "reference not present"
    lib, version, renderer = _lib()
    shaders, shas = _shaders()
    manifest = dict(gl_version=version, gl_renderer=renderer, shaders=shas, vertex_distance={}, frames={})
    print(version, "|", renderer)
    files = [{}, {}]
    worst = {}
    for k, name in enumerate(surfel_cases.VERTEX_CASES):
        case = surfel_cases.vertex_case(name)
        written, cap = capture(lib, shaders, case)
        v = surfel_ref.vertex(case)
        assert written[v["visible"]].all(), f"{name}: the model draws a splat whose gl_Position the shader never wrote"
        sel = {key: (val[written] if isinstance(val, np.ndarray) else val) for key, val in v.items()}
        d = surfel_ref.gl_distances(sel, cap, case["width"], case["height"])
        vis = v["visible"][written]
        per = {key: float(val[vis].max()) for key, val in d.items()}
        manifest["vertex_distance"][name] = per
        for key, val in per.items():
            worst[key] = max(worst.get(key, 0.0), val)
        print(name, "written", int(written.sum()), "model draws", int(v["visible"].sum()), json.dumps(per))
        files[k // 4]["written_" + name], files[k // 4]["vs_" + name] = written, cap
    manifest["vertex_distance"]["worst"] = worst
    # (the designed case whose second surfel leaves gl_Position unwritten stays out of the GL frames: what GL then draws is undefined)
    framed = [("frame", n) for n in surfel_cases.FRAME_CASES] + [("designed", n) for n in surfel_cases.DESIGNED_CASES if n != "distance_reject"]
    for kind, name in framed:
        case, order, dest = (surfel_cases.frame_case if kind == "frame" else surfel_cases.designed_case)(name)
        img = draw(lib, shaders, case, order, dest)
        assert img[..., 3].any(), f"{name}: GL drew nothing"
        out = surfel_ref.render(case, order, **dest)
        clean = out["covered"] & ~out["ambiguous"]
        rop = surfel_ref.composite_rop8(out["vertex"], out["fragments"], case["width"], case["height"], dest.get("dest_rgba"))
        d32, d8 = np.abs(out["frame"].astype(int) - img.astype(int)), np.abs(rop.astype(int) - img.astype(int))
        manifest["frames"][name] = dict(fp32_worst=int(d32[clean].max()), fp32_equal=round(float((d32[clean] == 0).mean()), 6),
                                        rop8_worst=int(d8[clean].max()), rop8_equal=round(float((d8[clean] == 0).mean()), 6),
                                        uncovered_equal=bool(np.array_equal(img[~out["covered"]], out["frame"][~out["covered"]])))
        print(name, json.dumps(manifest["frames"][name]))
        files[1]["frame_" + name] = img
    files[0]["manifest"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), np.uint8)
    MGG._save(os.path.join(GOLDEN, "surfel_gl_ref.npz"), files[0])
    MGG._save(os.path.join(GOLDEN, "surfel_gl_ref2.npz"), files[1])


if __name__ == "__main__":
    main()
