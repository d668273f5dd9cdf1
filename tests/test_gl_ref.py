"""Raster parity PINNED to a real GL: tests/golden/gl_*_ref.npz hold what the reference's OWN, unmodified shader strings and its
blend state compute on Mesa's llvmpipe (OpenGL ES 3.2, oracle/make_golden_gl.py + oracle/gl_ref.c): transform feedback of the
vertex stage for the 12 raster cases and for ~4096 splats of a 1.1 M-splat scene (data-texture reads at the reference's texture
sizes and at high splat indices), the fragment shader at sampled varyings, and RGBA8 frames of one instanced draw with
NormalBlending.  CPU tier (this file): the C raster oracle and the CPU shim (raster_ref.npz) against GL.  GPU tier:
tests/test_gpu_gl_ref.py.  Stand-ins left: the three.js WebGLProgram prefix and the texel packing (oracle/texel_pack.h)."""
import json
import os

import numpy as np
import pytest

import gl_cases
import oracle
import raster_cases
from test_raster_ref import _from_shader, _oracle_camera

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GV = np.load(os.path.join(HERE, "gl_vertex_ref.npz"))
GH = np.load(os.path.join(HERE, "gl_vertex_high_ref.npz"))
GF = {**dict(np.load(os.path.join(HERE, "gl_frames_ref.npz"))), **dict(np.load(os.path.join(HERE, "gl_frames2_ref.npz")))}
SR = np.load(os.path.join(HERE, "raster_ref.npz"))
FRAME_MANIFEST = json.loads(bytes(GF["manifest"]).decode())

# Tripwire of the C oracle's rop8 mode (floor(x * 255 + 0.5) after every splat, on the fp32 colour) against GL's RGBA8 blend: the
# worst channel difference per frame as recorded by oracle/make_golden_gl.py (the manifest's rop8_oracle_vs_gl).  llvmpipe
# converts the fragment's colour to unorm8 BEFORE it blends ("What a real GL showed"): the two RGBA8 rules sit up
# to this far apart; the derived bound below holds GL to the exact composite.
ROP8_ORACLE_VS_GL_MAX = {"rop_sh0": 6, "rop_sh2": 6, "rop_sh1_half": 5, "antialiased": 4, "orthographic": 6, "translucent": 20,
                         "edges_near_far": 6, "dst_depth32f": 5, "dst_depth24": 5}
# Splats whose accept / reject decision differs between the C oracle and GL, by case: (index, reason).  Empty: none differ.
VERTEX_EXCEPTIONS = {}


def gl_vertex(res8):
    """gl_vertex_ref layout [n, 4, 8] -> raster_ref's [n, 4, 10] with vPosition left NaN, and a mask of the splats whose shader
    returned before writing gl_Position (its value is undefined in GL; llvmpipe leaves w = 0, which GL clips whole)."""
    n = res8.shape[0]
    out = np.full((n, 4, 10), np.nan, np.float32)
    out[:, :, 0:8] = res8
    undefined = ~(res8[:, :, 3] == 1.0).all(axis=1)
    out[undefined, :, 0:4] = np.nan
    return out, undefined


def _check_vertex(name, case, res, idx=None):
    """test_raster_ref.test_c_oracle_vertex_stage_matches_the_reference_shader's checks and tolerances, GL as the reference."""
    drawn, centre, b1, b2, colour = _from_shader(res, case["uniforms"]["viewport"])
    sel = slice(None) if idx is None else idx
    sh = None
    if case["sh_stored"]:
        sh = case["sh_u8"].astype(np.float32) if case["sh8"] else case["sh_sampled"][sel]
    o = oracle.project(_oracle_camera(case), case["centers"][sel], case["cov"][sel], case["rgba"][sel], sh,
                       scene_indexes=None if case["scene_idx"] is None else case["scene_idx"][sel])
    vis = o["visible"] == 1
    exc = np.zeros(vis.shape[0], bool)
    for i, _reason in VERTEX_EXCEPTIONS.get(name, ()):
        exc[i] = True
    assert drawn.sum() > 100
    np.testing.assert_array_equal(vis[~exc], drawn[~exc], err_msg=f"{name}: accept / reject decisions differ from GL's")
    k = drawn & vis
    np.testing.assert_allclose(o["cx"][k], centre[k, 0], rtol=0, atol=2e-3)
    np.testing.assert_allclose(o["cy"][k], centre[k, 1], rtol=0, atol=2e-3)
    for col, ref in (("b1x", b1[:, 0]), ("b1y", b1[:, 1]), ("b2x", b2[:, 0]), ("b2y", b2[:, 1])):
        np.testing.assert_allclose(o[col][k], ref[k], rtol=2e-4, atol=1e-4 * max(case["uniforms"]["viewport"]) / 100)
    tol = 2e-4 if name == "dynamic" else 3e-6
    for ch, col in enumerate("rgba"):
        np.testing.assert_allclose(o[col][k], colour[k, ch], rtol=0, atol=tol)


@pytest.mark.parametrize("name", raster_cases.CASES)
def test_c_oracle_vertex_stage_matches_gl(name):
    case = raster_cases.make_case(name)
    res, _ = gl_vertex(GV["vs_" + name])
    _check_vertex(name, case, res)


@pytest.mark.parametrize("name", list(gl_cases.HIGH_CASES))
def test_c_oracle_vertex_stage_matches_gl_at_high_splat_indices(name):
    """Texture reads at the reference's sizes (SH: 4096 x 2048 RGBA16F, texel indices to 6.6 M) and, with fp32 covariances,
    getDataUVF's float(sIndex) * 1.5, for splats about every power of two up to 2^20 and the last ones of 1.1 M."""
    idx = GH["index"]
    np.testing.assert_array_equal(idx, gl_cases.high_indices())
    assert idx.max() == gl_cases.HIGH_N - 1 and idx.size >= 4000
    case = gl_cases.high_case(name)
    res, _ = gl_vertex(GH["vs_" + name])
    _check_vertex(name, case, res, idx)


@pytest.mark.parametrize("name", raster_cases.CASES)
def test_cpu_shim_matches_gl(name):
    """The missing test of oracle/glsl_shim.hpp: its execution of the same shader strings (raster_ref.npz) against GL, quantity by
    quantity, at the C oracle's tolerances (measured: gl_Position within 4.8e-7, vColor within 3.6e-7)."""
    case = raster_cases.make_case(name)
    gl, undefined = gl_vertex(GV["vs_" + name])
    shim = SR["vs_" + name]
    # the shader's early `return` (eigenValue2 <= 0) leaves gl_Position undefined: the shim writes NaN, GL clips what it got
    np.testing.assert_array_equal(undefined, ~np.isfinite(shim[:, :, 0:4]).all(axis=(1, 2)))
    vp = case["uniforms"]["viewport"]
    d_gl, c_gl, b1_gl, b2_gl, col_gl = _from_shader(gl, vp)
    d_sh, c_sh, b1_sh, b2_sh, col_sh = _from_shader(shim, vp)
    np.testing.assert_array_equal(d_gl, d_sh)
    k = d_gl
    np.testing.assert_allclose(c_sh[k], c_gl[k], rtol=0, atol=2e-3)
    np.testing.assert_allclose(b1_sh[k], b1_gl[k], rtol=2e-4, atol=1e-4 * max(vp) / 100)
    np.testing.assert_allclose(b2_sh[k], b2_gl[k], rtol=2e-4, atol=1e-4 * max(vp) / 100)
    np.testing.assert_allclose(col_sh[k], col_gl[k], rtol=0, atol=2e-4 if name == "dynamic" else 3e-6)
    np.testing.assert_allclose(shim[k][:, :, 0:8], gl[k][:, :, 0:8], rtol=0, atol=1e-6)


def test_cpu_shim_fragment_rule_matches_gl():
    """The discard edge and the colour are exact.  The opacity exp(-0.5 A) * vColor.a: GLSL ES 3.00 §4.5.1 allows exp() an error
    of (3 + 2 |x|) ULP at highp, one more ULP for the product; llvmpipe's exp sits up to 4.1e-7 relative from the shim's (libm)."""
    col, disc = GV["fs_color"], GV["fs_discard"].astype(bool)
    np.testing.assert_array_equal(disc, SR["fs_discard"].astype(bool))
    keep = ~disc
    np.testing.assert_array_equal(col[keep, :3], SR["fs_color"][keep, :3])
    vp, _ = raster_cases.fragment_samples()
    x = 0.5 * (vp[keep] ** 2).sum(axis=1).astype(np.float64)
    ulps = 3.0 + 2.0 * x + 1.0
    rel = np.abs(col[keep, 3].astype(np.float64) - SR["fs_color"][keep, 3]) / np.abs(SR["fs_color"][keep, 3].astype(np.float64))
    assert (rel <= ulps * 2.0 ** -23).all(), float((rel / (ulps * 2.0 ** -23)).max())
    assert rel.max() <= 5e-7                  # what llvmpipe does: a tripwire well inside the spec's bound


def test_gl_manifest_describes_the_shaders_of_raster_ref():
    meta = json.loads(bytes(SR["meta"]).decode())
    for m in (json.loads(bytes(GV["manifest"]).decode()), FRAME_MANIFEST):
        assert m["gl_renderer"].startswith("llvmpipe") and "OpenGL ES 3" in m["gl_version"]
        for b, s in m["shaders"].items():
            assert s["vert_sha256"] == meta[b]["vert_sha256"] and s["frag_sha256"] == meta[b]["frag_sha256"]


def _oracle_frames(case, rop8, bounds=None, gl_depth=False):
    """The C oracle's frame of a frame case.  A DEPTH_COMPONENT24 destination is compared as the engine does (exact
    round(z (2^24 - 1)), mode 1) or, gl_depth=True, as llvmpipe converts (the product in fp32, mode 2)."""
    ocam = _oracle_camera(case)
    sh = case["sh_sampled"] if case["sh_stored"] else None
    mode = (2 if gl_depth else 1) if case["depth_format"] else 0
    (fb, amb), = oracle.render_windows(ocam, case["centers"], case["cov"], case["rgba"], sh, case["order"],
                                       windows=[(0, 0, case["w"], case["h"])], rop8=rop8, depth=case["depth"],
                                       depth_unorm24=mode, dst_rgba=case["dst"], error_bounds=bounds)[0]
    return fb, amb.astype(bool)


def q8(fb):
    return np.floor(np.clip(fb, 0, 1) * 255.0 + 0.5).astype(np.int32)


def rop8_gate_excess(x, gl, ref8, slack=1):
    """How far an RGBA8 frame x sits beyond the per-pixel gate |x - GL| <= |rop8 oracle - GL| + slack (ints, [h, w, c])."""
    return np.abs(x.astype(np.int32) - gl) - (np.abs(ref8 - gl) + slack)


def footprints(case):
    """Per pixel, from the C oracle's vertex stage: whether some drawn splat's ellipse (A <= 8) holds the pixel centre, and the
    largest single-fragment alpha exp(-0.5 A) * a there (no destination: every fragment passes)."""
    o = oracle.project(_oracle_camera(case), case["centers"], case["cov"], case["rgba"],
                       case["sh_sampled"] if case["sh_stored"] else None, order=case["order"])
    H, W = case["h"], case["w"]
    covered = np.zeros((H, W), bool)
    amax = np.zeros((H, W), np.float32)
    for r in o[o["visible"] == 1]:
        b1, b2 = np.array([r["b1x"], r["b1y"]], np.float64), np.array([r["b2x"], r["b2y"]], np.float64)
        ex, ey = np.hypot(b1[0], b2[0]), np.hypot(b1[1], b2[1])
        x0, x1 = max(int(np.floor(r["cx"] - ex - 1)), 0), min(int(np.ceil(r["cx"] + ex + 1)), W)
        y0, y1 = max(int(np.floor(r["cy"] - ey - 1)), 0), min(int(np.ceil(r["cy"] + ey + 1)), H)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        dx, dy = xx + 0.5 - r["cx"], yy + 0.5 - r["cy"]
        u = (dx * b1[0] + dy * b1[1]) / (b1 @ b1)
        v = (dx * b2[0] + dy * b2[1]) / (b2 @ b2)
        A = 8.0 * (u * u + v * v)
        inside = A <= 8.0
        covered[y0:y1, x0:x1] |= inside
        amax[y0:y1, x0:x1] = np.maximum(amax[y0:y1, x0:x1], np.where(inside, np.exp(-0.5 * A) * r["a"], 0.0))
    return covered, amax


@pytest.mark.parametrize("name", gl_cases.FRAMES)
def test_rop8_oracle_matches_gl_frames(name):
    """The rop8 oracle against GL's RGBA8 blend: per channel the recorded agreement (equal fraction no lower, worst difference no
    higher than the tripwire) and the same covered pixels."""
    case = gl_cases.make_frame(name)
    assert case["order_sha256"] == FRAME_MANIFEST["order_sha256"][name], f"{name}: the scene or its sort changed"
    gl = GF["frame_" + name].astype(np.int32)
    fb8, amb = _oracle_frames(case, rop8=True, gl_depth=True)
    ref8 = q8(fb8)
    d = np.abs(gl - ref8)
    rec = FRAME_MANIFEST["rop8_oracle_vs_gl"][name]
    for k, ch in enumerate("rgba"):
        assert (d[..., k] == 0).mean() >= rec[ch]["equal"] - 1e-6, (name, ch, float((d[..., k] == 0).mean()), rec[ch])
    assert d.max() <= ROP8_ORACLE_VS_GL_MAX[name], (name, int(d.max()))
    if case["dst"] is None:                  # coverage: GL writes a pixel where the per-splat-rounding target does, nowhere else
        cover_gl, cover_o = gl[..., 3] > 0, ref8[..., 3] > 0
        bad = (cover_gl != cover_o) & ~amb
        assert not bad.any(), f"{name}: {int(bad.sum())} pixels covered by one side only, e.g. {np.argwhere(bad)[:5].tolist()}"


def test_depth24_destination_decides_differently_from_depth32f():
    """The DEPTH_COMPONENT24 frame pins the unorm24 depth test: GL's two frames differ where the stored depth sits within a unorm24
    step below a splat's depth, and the oracle explains both.  llvmpipe forms z (2^24 - 1) in fp32 before it rounds, which can
    round across a level; the exact rule (the engine's, oracle mode 1) keeps different splats on some of those pixels."""
    a, b = GF["frame_dst_depth32f"].astype(np.int32), GF["frame_dst_depth24"].astype(np.int32)
    assert (a != b).any(axis=-1).sum() > 1000
    case = gl_cases.make_frame("dst_depth24")
    exact, llvm = q8(_oracle_frames(case, rop8=True)[0]), q8(_oracle_frames(case, rop8=True, gl_depth=True)[0])
    assert np.abs(llvm - b).max() <= ROP8_ORACLE_VS_GL_MAX["dst_depth24"]
    assert np.abs(exact - b).max() > 20, "the exact unorm24 rule now explains llvmpipe's frame: revisit DESIGN.md section 2"


@pytest.mark.parametrize("name", gl_cases.FRAMES)
def test_rop8_gate_rejects_a_blend_that_rounds_once(name):
    """The engine's GS_DRAW_ROP8 gate (tests/test_gpu_gl_ref.py: |engine - GL| <= |rop8 oracle - GL| + 1 per value) has power: the
    fp32 composite rounded once at the end, standing in for a kernel that rounds only there, fails it on every frame."""
    case = gl_cases.make_frame(name)
    gl = GF["frame_" + name].astype(np.int32)
    ref8 = q8(_oracle_frames(case, rop8=True)[0])
    once = q8(_oracle_frames(case, rop8=False)[0])
    assert rop8_gate_excess(ref8, gl, ref8).max() <= 0
    assert (rop8_gate_excess(once, gl, ref8) > 0).sum() >= 10, name


@pytest.mark.parametrize("name", gl_cases.FRAMES)
def test_fp32_oracle_bounds_gl_frames(name):
    """GL's RGBA8 frame against the exact (fp32) composite: within the derived per-pixel bound of a target that rounds after every
    splat (raster_oracle.c: e <- (1 - a) e + 0.5) plus llvmpipe's rounding of the fragment colour before it blends (recorded
    tripwire).  Coverage both ways against the oracle's footprint test (A <= 8 at the pixel centre): GL covers no pixel the
    footprints leave empty, and covers every pixel where some fragment's alpha rounds to at least one step."""
    case = gl_cases.make_frame(name)
    gl = GF["frame_" + name].astype(np.float32)
    bounds = []
    fb, amb = _oracle_frames(case, rop8=False, bounds=bounds, gl_depth=True)
    e = bounds[0]
    err = np.abs(gl - np.clip(fb, 0, 1) * 255.0)
    excess = (err - (e[..., None] + GL_SOURCE_SLACK[name]))[~amb]
    assert excess.max() <= 0.0, (name, float(excess.max()), float(err.max()), float(e.max()))
    if case["dst"] is None:
        covered, amax = footprints(case)
        bad = (gl[..., 3] > 0) & ~covered & ~amb
        assert not bad.any(), f"{name}: GL covers {int(bad.sum())} pixels the oracle's footprint test leaves empty"
        bad = (amax >= 0.6 / 255.0) & ~(gl[..., 3] > 0) & ~amb          # llvmpipe rounds a fragment's alpha to unorm8 first
        assert not bad.any(), f"{name}: GL leaves {int(bad.sum())} pixels empty that a fragment of alpha >= 0.6/255 covers"


# llvmpipe rounds the fragment's colour and alpha to unorm8 before it blends: beyond the per-splat 0.5 of the derived bound, a
# splat may move a channel further through its rounded colour and alpha.  Measured worst excess over e by frame,
# plus 0.25 as the tripwire.
GL_SOURCE_SLACK = {"rop_sh0": 0.80 + 0.25, "rop_sh2": 0.51 + 0.25, "rop_sh1_half": 0.75 + 0.25, "antialiased": 1.18 + 0.25,
                   "orthographic": 0.92 + 0.25, "translucent": 0.0 + 0.25, "edges_near_far": 0.68 + 0.25, "dst_depth32f": 1.24 + 0.25,
                   "dst_depth24": 1.24 + 0.25}
