"""oracle/make_golden_gl.py — records what the REFERENCE's own, unmodified shader strings and blend state compute on a real GLES 3
rasteriser (Mesa llvmpipe, driven headless by oracle/gl_ref.c) into three fixtures.  Runs only where /root/reference, Node and
swrast_dri.so exist (`make -C oracle glref` first); the tests read the fixtures alone.

  tests/golden/gl_vertex_ref.npz       transform feedback of gl_Position and vColor for every (splat, quad corner) of the 12
                                       tests/raster_cases.py cases ([n, 4, 8]: raster_ref.npz's layout without vPosition, which
                                       the generator checks is corner * sqrt(8) everywhere); the reference's fragment shader at
                                       raster_cases.fragment_samples(); a JSON manifest.
  tests/golden/gl_vertex_high_ref.npz  the same captures for about 4096 splats of a 1.1 M-splat SH-2 scene (tests/gl_cases.py),
                                       with fp32 and with fp16 covariances, and their splat indices.
  tests/golden/gl_frames_ref.npz,
  tests/golden/gl_frames2_ref.npz      RGBA8 frames (glReadPixels, row 0 = bottom) of tests/gl_cases.FRAMES, one instanced draw
                                       each with SplatMaterial3D's blend / depth state (split in two files by size), the sha-256 of every
                                       sorted order and the measured distance of the C oracle's rop8 mode to each frame.

The shader strings come from oracle/shader_dump.mjs exactly as for oracle/make_golden_raster.py (scratch copies under
oracle/_ref/gl/); their sha-256 must equal those recorded in raster_ref.npz, so both fixtures describe the same shaders.
A second run writes byte-identical files.
usage: make -C oracle glref && python -m oracle.make_golden_gl"""
import ctypes as C
import hashlib
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gl_cases  # noqa: E402
import raster_cases  # noqa: E402

import oracle  # noqa: E402
from oracle import make_golden_raster as MGR  # noqa: E402

REF_SRC = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden")
SQRT8 = np.float32(np.sqrt(np.float32(8.0)))
LP_NUM_THREADS = "4"          # what oracle/gl_ref.c sets


def _lib():
    so = os.path.join(ROOT, "oracle", "_ref", "libglref.so")
    assert os.path.exists(so), "run `make -C oracle glref` first (needs the reference and swrast_dri.so)"
    lib = C.CDLL(so)
    v, r = C.create_string_buffer(256), C.create_string_buffer(256)
    rc = lib.glref_init(v, r, 256)
    assert rc == 0, f"glref_init: {rc}"
    return lib, v.value.decode(), r.value.decode()


def _shaders():
    scratch = os.path.join(ROOT, "oracle", "_ref", "gl")
    os.makedirs(scratch, exist_ok=True)
    builds = raster_cases.shader_builds()
    json.dump([dict(name=k, **v) for k, v in builds.items()], open(os.path.join(scratch, "perms.json"), "w"))
    subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(ROOT, "oracle", "three_loader.mjs"),
                           os.path.join(ROOT, "oracle", "shader_dump.mjs"), REF_SRC, scratch, os.path.join(scratch, "perms.json")],
                          cwd=os.path.join(ROOT, "oracle"), stdout=subprocess.DEVNULL)
    recorded = json.loads(bytes(np.load(os.path.join(GOLDEN, "raster_ref.npz"))["meta"]).decode())
    out, shas = {}, {}
    for name in builds:
        vert, frag = open(os.path.join(scratch, name + ".vert")).read(), open(os.path.join(scratch, name + ".frag")).read()
        shas[name] = dict(vert_sha256=hashlib.sha256(vert.encode()).hexdigest(), frag_sha256=hashlib.sha256(frag.encode()).hexdigest())
        assert shas[name]["vert_sha256"] == recorded[name]["vert_sha256"], f"{name}: vertex shader differs from raster_ref.npz's"
        assert shas[name]["frag_sha256"] == recorded[name]["frag_sha256"], f"{name}: fragment shader differs from raster_ref.npz's"
        out[name] = (vert.encode(), frag.encode())
    return out, shas


def capture(lib, shaders, case, splat_index=None):
    """[count, 4, 10] transform-feedback captures of the case's splats (or of `splat_index`)."""
    sc, u, _keep = MGR.harness_inputs(case)
    vert, frag = shaders[case["build"]]
    if splat_index is None:
        count, idx = sc.count, None
    else:
        idx = np.ascontiguousarray(splat_index, np.uint32)
        count = idx.shape[0]
    out = np.zeros((count, 4, 10), np.float32)
    rc = lib.glref_capture_vertices(vert, frag, C.byref(sc), C.byref(u), idx.ctypes.data_as(C.c_void_p) if idx is not None else None,
                                    C.c_uint32(count), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, f"glref_capture_vertices: {rc}"
    return out


def draw(lib, shaders, case):
    sc, u, _keep = MGR.harness_inputs(case)
    vert, frag = shaders[case["build"]]
    w, h = case["w"], case["h"]
    order = np.ascontiguousarray(case["order"], np.uint32)
    depth = None if case["depth"] is None else np.ascontiguousarray(case["depth"], np.float32)
    dst = None if case["dst"] is None else np.ascontiguousarray(case["dst"], np.uint8)
    out = np.zeros((h, w, 4), np.uint8)
    rc = lib.glref_draw_frame(vert, frag, C.byref(sc), C.byref(u), order.ctypes.data_as(C.c_void_p), C.c_uint32(order.shape[0]),
                              C.c_int(w), C.c_int(h), depth.ctypes.data_as(C.c_void_p) if depth is not None else None,
                              C.c_int(case["depth_format"]), dst.ctypes.data_as(C.c_void_p) if dst is not None else None,
                              out.ctypes.data_as(C.c_void_p))
    assert rc == 0, f"glref_draw_frame: {rc}"
    return out


def fragments(lib, shaders):
    vp, vc = raster_cases.fragment_samples()
    col = np.zeros((vp.shape[0], 4), np.float32)
    disc = np.zeros(vp.shape[0], np.uint8)
    rc = lib.glref_run_fragment(shaders["base0"][1], C.c_uint32(vp.shape[0]), vp.ctypes.data_as(C.c_void_p),
                                vc.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), disc.ctypes.data_as(C.c_void_p))
    assert rc == 0, f"glref_run_fragment: {rc}"
    return col, disc


def _vertex_layout(res):
    """[n, 4, 10] -> [n, 4, 8]: vPosition must be corner * sqrt(8) wherever the shader reached its end (w == 1, not the
    rejection's (0, 0, 2, 1))."""
    done = (res[:, :, 3] == 1.0).all(axis=1) & ~(res[:, :, 2] == 2.0).all(axis=1)
    corners = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], np.float32) * SQRT8
    assert np.array_equal(res[done][:, :, 8:10], np.broadcast_to(corners, (int(done.sum()), 4, 2)))
    return np.ascontiguousarray(res[:, :, 0:8])


def rop8_agreement(case, gl):
    """GL's frame against the C oracle's rop8 mode (floor(x * 255 + 0.5) after every splat; a unorm24 destination depth converted
    as llvmpipe converts it, oracle mode 2): per channel the fraction of equal values, the max difference and the pixels that
    differ."""
    import test_raster_ref
    ocam = test_raster_ref._oracle_camera(case)
    sh = case["sh_sampled"] if case["sh_stored"] else None
    (fb8, _), = oracle.render_windows(ocam, case["centers"], case["cov"], case["rgba"], sh, case["order"],
                                      windows=[(0, 0, case["w"], case["h"])], rop8=True, depth=case["depth"],
                                      depth_unorm24=2 if case["depth_format"] else 0, dst_rgba=case["dst"])[0]
    ref8 = np.floor(np.clip(fb8, 0, 1) * 255.0 + 0.5).astype(np.int32)
    d = np.abs(gl.astype(np.int32) - ref8)
    return {ch: dict(equal=round(float((d[..., k] == 0).mean()), 6), max=int(d[..., k].max()), pixels=int((d[..., k] != 0).sum()))
            for k, ch in enumerate("rgba")}


def _save(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())
    data = buf.getvalue()
    assert len(data) <= 1 << 20, f"{path}: {len(data)} bytes is over the 1 MiB limit of a committed file"
    with open(path, "wb") as f:
        f.write(data)
    print(f"wrote {os.path.relpath(path, ROOT)} ({len(data)} bytes)")


def main():
    assert os.path.isdir(REF_SRC), "reference not present"
    lib, version, renderer = _lib()
    shaders, shas = _shaders()
    manifest = dict(gl_version=version, gl_renderer=renderer, lp_num_threads=LP_NUM_THREADS, shaders=shas)
    print(version, "|", renderer)

    vx = {}
    for cname in raster_cases.CASES:
        case = raster_cases.make_case(cname)
        vx["vs_" + cname] = _vertex_layout(capture(lib, shaders, case))
    col, disc = fragments(lib, shaders)
    vx["fs_color"], vx["fs_discard"] = col, disc
    vx["manifest"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), np.uint8)
    _save(os.path.join(GOLDEN, "gl_vertex_ref.npz"), vx)

    hi = {"index": gl_cases.high_indices()}
    for name in gl_cases.HIGH_CASES:
        case = gl_cases.high_case(name)
        hi["vs_" + name] = _vertex_layout(capture(lib, shaders, case, hi["index"]))
    _save(os.path.join(GOLDEN, "gl_vertex_high_ref.npz"), hi)

    fr, agree, shas_order = {}, {}, {}
    for name in gl_cases.FRAMES:
        case = gl_cases.make_frame(name)
        img = draw(lib, shaders, case)
        assert img[..., 3].any(), f"{name}: GL drew nothing"
        fr["frame_" + name] = img
        shas_order[name] = case["order_sha256"]
        agree[name] = rop8_agreement(case, img)
        print(name, json.dumps(agree[name]))
    manifest_f = dict(manifest, order_sha256=shas_order, rop8_oracle_vs_gl=agree)
    fr["manifest"] = np.frombuffer(json.dumps(manifest_f, sort_keys=True).encode(), np.uint8)
    # two files: each within the 1 MiB limit of a committed file
    second = {"frame_" + n for n in gl_cases.FRAMES[5:]}
    _save(os.path.join(GOLDEN, "gl_frames_ref.npz"), {k: v for k, v in fr.items() if k not in second})
    _save(os.path.join(GOLDEN, "gl_frames2_ref.npz"), {k: v for k, v in fr.items() if k in second})


if __name__ == "__main__":
    main()
