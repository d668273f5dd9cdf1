"""-m gpu: the HIP vertex stage on the COMBINED shader permutations (tests/raster_combo_cases.py), held to what the reference's own
GLSL computed for them (tests/golden/raster_combo_ref.npz, made by oracle/make_golden_raster.py --combos; only the .npz is read).
One mesh per case, one context for the module.  Per case:
  records      drawn in upload order, the vertex-stage records pass test_raster_ref.check_engine_records unchanged, and the mesh says
               that the shader-permutation (EXT) instance of k_project ran;
  depth        drawn again over a float destination depth that hides nothing, the DEPTH instance of the same body leaves the visible
               mask, the slots, the rects and the records of the first draw bit for bit;
  strips       strips of two tile rows tile the full frame bit for bit (the dynamic cases take the strip pre-test's fall-back to the
               size clamp);
  frame        in sorted order the frame is within helpers.compare_frames' bar of oracle.render with the same per-scene uniforms."""
import os

import numpy as np
import pytest

import helpers
import oracle
import raster_combo_cases as rcc
from gaussiansplats3d_amd import Context
from gaussiansplats3d_amd import _lib as L
from test_gpu_permutations import _order, _strips_equal_frame
from test_raster_ref import _from_shader, _oracle_camera, check_engine_records, engine_mesh

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_combo_ref.npz"))
FAR_PLANE = np.ones((rcc.H, rcc.W), dtype=np.float32)
EXT, DEPTH = 1, 2                                              # bits of view_share()["instance"]: gs_mesh_debug_read(what = 6) word 3


@pytest.fixture(scope="module")
def meshes():
    """name -> (case, mesh): built on first use, kept for the module's four tests of the case."""
    ctx = Context(0)
    made = {}

    def get(name):
        if name not in made:
            case = rcc.make_case(name)
            made[name] = (case, engine_mesh(ctx, case))
        return made[name]
    yield get
    for _, mesh in made.values():
        mesh.dispose()
    ctx.close()


def draw_in_upload_order(case, mesh, destination_depth=None):
    """One full-frame draw in upload order; the vertex stage's outputs and the instance that made them."""
    n = case["scene"].count
    mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)
    if destination_depth is not None:
        mesh.set_destination(depth=destination_depth)
    try:
        mesh.render()
        recs, rects, vis = mesh.debug_records()
        slots = np.empty(n, dtype=np.uint32)
        L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 9, slots.ctypes.data, n))
        return dict(recs=recs, rects=rects, vis=vis, slots=slots, instance=mesh.view_share()["instance"])
    finally:
        if destination_depth is not None:
            mesh.set_destination()


def observed(case, res, recs, on_screen):
    """The worst differences check_engine_records bounds, as numbers: (centre px, basis relative to its length, colour)."""
    _, centre, b1, b2, colour = _from_shader(res, case["uniforms"]["viewport"])
    k, f = on_screen, recs.view(np.float32)
    d_centre = float(np.abs(f[k, 0:2] - centre[k]).max())
    d_basis = 0.0
    for col, b in ((2, b1), (4, b2)):
        want = 2.4022448 * b[k] / (b[k] ** 2).sum(axis=1)[:, None]
        d_basis = max(d_basis, float((np.abs(f[k, col:col + 2] - want).max(axis=1) / np.sqrt((want ** 2).sum(axis=1))).max()))
    got = np.stack([(recs[k, 6] & 0xFFFF), (recs[k, 6] >> 16), (recs[k, 7] & 0xFFFF), (recs[k, 7] >> 16)], axis=1) / 65535.0
    return d_centre, d_basis, float(np.abs(got - np.clip(colour[k], 0, 1)).max())


@pytest.mark.parametrize("name", rcc.CASES)
def test_records_match_the_reference_shader(meshes, name):
    case, mesh = meshes(name)
    d = draw_in_upload_order(case, mesh)
    assert d["instance"] & EXT and not d["instance"] & DEPTH, d["instance"]
    drawn = _from_shader(G["vs_" + name], case["uniforms"]["viewport"])[0]
    centre, basis, colour = observed(case, G["vs_" + name], d["recs"], d["vis"] & drawn)
    print(f"{name}: the shader draws {int(drawn.sum())}, the engine {int(d['vis'].sum())}; worst centre {centre:.2e} px (gate 3e-3), "
          f"basis {basis:.2e} of its length (gate 5e-4), colour {colour:.2e} (gate 2e-5)")
    check_engine_records(case, G["vs_" + name], d["recs"], d["vis"])
    gone = rcc.scene_rejected(case)[case["scene_idx"]]          # no splat of a scene the shader rejects whole is drawn
    assert not d["vis"][gone].any()


@pytest.mark.parametrize("name", rcc.CASES)
def test_depth_instance_draws_the_same_records(meshes, name):
    case, mesh = meshes(name)
    plain, deep = draw_in_upload_order(case, mesh), draw_in_upload_order(case, mesh, FAR_PLANE)
    assert plain["instance"] & EXT and not plain["instance"] & DEPTH, plain["instance"]
    assert deep["instance"] & EXT and deep["instance"] & DEPTH, deep["instance"]
    v = plain["vis"]
    assert v.sum() > 80
    assert np.array_equal(deep["vis"], v) and np.array_equal(deep["slots"], plain["slots"])
    assert np.array_equal(deep["rects"][v], plain["rects"][v])
    same = (deep["recs"][v] == plain["recs"][v]).all(axis=0)
    assert same.all(), ("record words that differ", np.flatnonzero(~same).tolist())


@pytest.mark.parametrize("name", rcc.CASES)
def test_strips_tile_the_frame(meshes, name):
    case, mesh = meshes(name)
    n = case["scene"].count
    mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)
    _strips_equal_frame(mesh, case["camera"], name)


@pytest.mark.parametrize("name", rcc.CASES)
def test_frame_matches_the_raster_oracle(meshes, name):
    case, mesh = meshes(name)
    order = _order(case["scene"], case["camera"])             # a fixed depth-like order: both sides draw it
    mesh.update_render_indexes(order, case["scene"].count)
    got, _ = mesh.render()
    sh = None
    if case["sh_stored"]:
        sh = case["sh_u8"].astype(np.float32) if case["sh8"] else case["sh_sampled"]
    fb, q, amb, frags = oracle.render(_oracle_camera(case), case["centers"], case["cov"], case["rgba"], sh, order,
                                      scene_indexes=case["scene_idx"])
    assert frags > 1000
    print(helpers.compare_frames(got, fb, amb, name))
