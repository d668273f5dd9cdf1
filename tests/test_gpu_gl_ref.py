"""-m gpu: the engine against what a real GL (Mesa llvmpipe) computed from the reference's own shader strings and blend state
(tests/golden/gl_*_ref.npz, see tests/test_gl_ref.py): the HIP vertex stage against transform feedback, including splat indices
up to 1.1 M at the reference's texture sizes; GS_DRAW_ROP8 / GS_DRAW_ROP8_FULL and the default fp32 draw against GL's RGBA8 frames,
with and without a destination (gs_mesh_set_destination) in both depth formats.  Reads only tests/golden/."""
import numpy as np
import pytest

import gl_cases
import raster_cases
from gaussiansplats3d_amd import Context
from test_gl_ref import GF, GH, GL_SOURCE_SLACK, GV, _oracle_frames, gl_vertex, q8, rop8_gate_excess
from test_gpu_crops import ENGINE_SLACK
from test_gpu_crops import _write_report
from test_raster_ref import check_engine_records, engine_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", raster_cases.CASES)
def test_hip_vertex_stage_matches_gl(ctx, name):
    case = raster_cases.make_case(name)
    n = case["scene"].count
    mesh = engine_mesh(ctx, case)
    mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)
    mesh.render()
    recs, _, on_screen = mesh.debug_records()
    check_engine_records(case, gl_vertex(GV["vs_" + name])[0], recs, on_screen)
    mesh.dispose()


@pytest.mark.parametrize("name", list(gl_cases.HIGH_CASES))
def test_hip_vertex_stage_matches_gl_at_high_splat_indices(ctx, name):
    case = gl_cases.high_case(name)
    n = case["scene"].count
    idx = GH["index"]
    mesh = engine_mesh(ctx, case)
    mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)
    mesh.render()
    recs, _, on_screen = mesh.debug_records()
    check_engine_records(case, gl_vertex(GH["vs_" + name])[0], recs[idx], on_screen[idx])
    mesh.dispose()


def _frame_mesh(ctx, case):
    mesh = engine_mesh(ctx, case)
    if case["dst"] is not None:
        mesh.set_destination(depth=case["depth"], rgba=case["dst"], depth_unorm24=bool(case["depth_format"]))
    mesh.update_render_indexes(case["order"], case["scene"].count)
    return mesh


@pytest.mark.parametrize("name", gl_cases.FRAMES)
def test_rop8_draw_matches_gl_frames(ctx, name):
    """GS_DRAW_ROP8_FULL per value no further from GL than the rop8 oracle plus one step (|engine - GL| <= |oracle - GL| + 1); a
    blend that rounds once at the end fails this on every frame (test_gl_ref.test_rop8_gate_rejects_a_blend_that_rounds_once).
    GS_DRAW_ROP8 the same on colour, its alpha with the documented <= 2-step exception on top (tile_blend.hip).  The oracle keeps
    the engine's exact unorm24 rule for the DEPTH_COMPONENT24 destination."""
    case = gl_cases.make_frame(name)
    gl = GF["frame_" + name].astype(np.int32)
    ref8 = q8(_oracle_frames(case, rop8=True)[0])
    mesh = _frame_mesh(ctx, case)
    for full in (True, False):
        mesh.set_draw_mode(rop8=True, full=full)
        got, _ = mesh.render()
        ex = rop8_gate_excess(got, gl, ref8)
        assert ex[..., :3].max() <= 0, (name, full, int(ex[..., :3].max()), int((ex[..., :3] > 0).sum()))
        assert ex[..., 3].max() <= (0 if full else 2), (name, full, int(ex[..., 3].max()))
    mesh.dispose()


@pytest.mark.parametrize("name", gl_cases.FRAMES)
def test_fp32_draw_matches_gl_frames(ctx, name):
    """The default draw against GL's RGBA8 frame, as tests/test_gpu_crops.py gates it against the ROP-emulating oracle: within the
    derived per-pixel bound e of an RGBA8 target (plus llvmpipe's source rounding, test_gl_ref.GL_SOURCE_SLACK) plus ENGINE_SLACK,
    outside the oracle's discard-ambiguous pixels; and the worst pixel at most the recorded worst plus one step.  On the
    DEPTH_COMPONENT24 frame the pixels where llvmpipe's fp32 depth conversion keeps other splats than the exact rule are held to
    the exact-rule oracle instead (strict 1/255, as tests/test_gpu_depth.py)."""
    case = gl_cases.make_frame(name)
    gl = GF["frame_" + name].astype(np.float32)
    mesh = _frame_mesh(ctx, case)
    got, _ = mesh.render()
    bounds = []
    fb, amb = _oracle_frames(case, rop8=False, bounds=bounds)
    other = np.zeros(amb.shape, bool)
    if case["depth_format"]:
        fb_gl, _ = _oracle_frames(case, rop8=False, gl_depth=True)
        other = (np.abs(fb_gl - fb) > 0).any(axis=-1)
        strict = np.abs(got.astype(np.float32) - np.clip(fb, 0, 1) * 255.0)[other & ~amb]
        assert other.sum() > 100 and strict.max() <= 1.5, (int(other.sum()), float(strict.max()))
    d = np.abs(got.astype(np.float32) - gl)
    excess = (d - (bounds[0][..., None] + GL_SOURCE_SLACK[name] + ENGINE_SLACK))[~amb & ~other]
    worst = float(d[~other].max())
    _write_report(f"gl_fp32_{name}.json", {"frame": name, "engine_vs_gl_max": worst, "engine_vs_gl_mean": float(d[~other].mean()),
                                           "excess_over_bound": float(excess.max()), "pixels_held_to_exact_depth": int(other.sum())})
    print(f"{name}: engine fp32 vs GL: max {worst:.0f}, mean {d[~other].mean():.3f}, excess over the bound {excess.max():+.2f}")
    assert excess.max() <= 0.0, (name, float(excess.max()), worst)
    assert worst <= FP32_VS_GL_RECORDED_MAX[name] + 1, (name, worst, FP32_VS_GL_RECORDED_MAX[name])
    mesh.dispose()


# The worst pixel of the engine's fp32 draw against each GL frame (in 1/255), measured on an MI355X (DESIGN.md §2 lists the run):
# a tripwire beside the derived bound, which reaches 8-11/255 on these frames.
FP32_VS_GL_RECORDED_MAX = {"rop_sh0": 4, "rop_sh2": 4, "rop_sh1_half": 4, "antialiased": 3, "orthographic": 6, "translucent": 17,
                           "edges_near_far": 5, "dst_depth32f": 5, "dst_depth24": 5}
