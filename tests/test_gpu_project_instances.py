"""-m gpu: all 24 instances of the vertex stage, k_project<EXT, MODE, DEPTH, NARROW> (csrc/project.hip), held to the shader goldens and
to each other.  tests/project_instance_cases.py plans the matrix - which scene, switch and destination launches which instance - and
tests/test_project_instances.py proves on the CPU that the plan reaches every instance and that its poses have dead storage blocks.

Every cell is one draw of a fresh 2000-splat mesh at 512 x 288; after it the mesh says which kernel it launched
(view_share: block_test, instance) and hands out the stage's outputs (debug_records, the slots of what = 9, bin_word_narrow and,
with a destination, debug_depths).  Per case:
  a  every cell ran the instance the plan names;
  b  at the golden pose every cell passes test_raster_ref.check_engine_records against the reference shader's outputs - the gate,
     with the tolerances, that the one default instance passes in test_raster_ref.py;
  c  within a pose every cell's visible mask, slots, rects, records, frame statistics and frame equal the reference cell's bit for
     bit (MODE 2, no destination, the 8-byte word: no block test at all - so the block tests dropped nothing that draws);
  d  the neutral EXT cases draw bit for bit what their non-EXT base scene draws (identity transforms: equal as values, -0 == +0);
  e  at the inside pose (and from the side, for the orthographic case) MODE 0 and MODE 1 see storage blocks without a visible splat
     next to blocks that are nearly all visible; the accept set is within the C oracle's and what is dropped is thin or outside;
  f  a strip of the inside pose is the full frame's visible set cut to its rows, rects clamped, again equal across instances;
  g  the window depths: the float plane within twice the forward error bound of the fp32 evaluation of the golden's
     gl_Position.z, the 24-bit plane the kernel's rounding rule applied to the float plane's value, both equal across MODE and NARROW.
"""
import numpy as np
import pytest

import oracle
import project_instance_cases as pic
import raster_cases
from gaussiansplats3d_amd import Context
from gaussiansplats3d_amd import _lib as L
from test_bin_word import word
from test_raster_ref import G, _oracle_camera, check_dropped_splats_miss_the_frame, check_engine_records, engine_mesh

pytestmark = pytest.mark.gpu
FAR_PLANE = np.ones((pic.H, pic.W), dtype=np.float32)          # the destination depth of the DEPTH cells: nothing is occluded
FLOAT_FIELDS = slice(0, 6)                                      # SplatRec: cx, cy, ax, ay, bx, by as floats, then two colour words


@pytest.fixture(scope="module")
def contexts():
    """(a context that chooses the look-up word, a context created under the switch that forces the 8-byte one, the patcher): the
    pattern of test_gpu_bin_word.py.  draw_cell sets the switch around the draws of the second."""
    mp = pytest.MonkeyPatch()
    a = Context(0)
    mp.setenv(pic.WIDE_SWITCH, "1")
    b = Context(0)
    mp.delenv(pic.WIDE_SWITCH)
    yield a, b, mp
    mp.undo()
    a.close()
    b.close()


def narrow_of(tiles_x, tiles_y, switch):
    return word(tiles=(tiles_x, tiles_y), switch=switch).narrow


def draw_cell(contexts, case, cell, tile_rows=None):
    """One cell: a fresh mesh created, filled and drawn under the cell's switches; everything the checks read."""
    mode_setting, depth, wide = cell
    a, b, mp = contexts
    switches = [s for s in (pic.MODE_SWITCH[mode_setting], pic.WIDE_SWITCH if wide else None) if s]
    for s in switches:
        mp.setenv(s, "1")
    try:
        mesh = engine_mesh(b if wide else a, case)
        n = case["scene"].count
        mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)
        if depth != "none":
            mesh.set_destination(depth=FAR_PLANE, depth_unorm24=depth == "unorm24")
        frame, st = mesh.render(tile_rows=tile_rows)
        recs, rects, vis = mesh.debug_records()
        slots = np.empty(n, dtype=np.uint32)
        L.check(mesh.lib.gs_mesh_debug_read(mesh.handle, 9, slots.ctypes.data, n))
        share = mesh.view_share()
        out = dict(frame=frame, stats=(int(st.visible_splats), int(st.tiles16), int(st.tile_entries)), recs=recs, rects=rects, vis=vis,
                   slots=slots, block_test=share["block_test"], instance=share["instance"], narrow=mesh.bin_word_narrow(),
                   z=mesh.debug_depths() if depth != "none" else None, positions=mesh.debug_cull_planes()[2])
        mesh.dispose()
    finally:
        for s in switches:
            mp.delenv(s)
    return out


def check_same_draw(got, ref, where, frame=True):
    """(c): bit for bit the same vertex-stage outputs, statistics and frame."""
    assert np.array_equal(got["vis"], ref["vis"]), where
    assert np.array_equal(got["slots"], ref["slots"]), where
    v = ref["vis"]
    assert np.array_equal(got["rects"][v], ref["rects"][v]), where
    same = (got["recs"][v] == ref["recs"][v]).all(axis=0)
    assert same.all(), (where, "record words that differ", np.flatnonzero(~same).tolist())
    if frame:
        assert got["stats"] == ref["stats"], (where, got["stats"], ref["stats"])
        assert got["frame"].tobytes() == ref["frame"].tobytes(), where


def check_instances(name, pcase, draws, strip, where):
    """(a), (c) and the cross-instance part of (g) for the cells of one case, pose and strip."""
    ref = draws[pic.REFERENCE_CELL]
    assert ref["vis"].any()
    for cell, d in draws.items():
        ext, mode, depth, narrow = pic.planned_instance(pcase, cell, strip, narrow_of)
        ran = (d["instance"] & 1, d["block_test"], (d["instance"] >> 1) & 1, (d["instance"] >> 2) & 1)
        assert ran == (ext, mode, depth, narrow), (where, cell, "planned", (ext, mode, depth, narrow), "ran", ran)
        assert d["narrow"] == bool(narrow), (where, cell)
        check_same_draw(d, ref, (where, cell))
    v = ref["vis"]
    for fmt in ("float", "unorm24"):
        planes = {cell: d["z"] for cell, d in draws.items() if cell[1] == fmt}
        first = next(iter(planes.values()))
        assert np.isfinite(first[v]).all() and np.isnan(first[~v]).all(), (where, fmt)
        for cell, z in planes.items():
            assert np.array_equal(z.view(np.uint32)[v], first.view(np.uint32)[v]), (where, cell, "window depths differ between instances")
    for (mode_setting, fmt, wide), d in draws.items():       # the 24-bit depth: the kernel's rounding rule on the float plane's value
        if fmt == "unorm24":
            zf = draws[(mode_setting, "float", wide)]["z"][v].astype(np.float64)
            assert np.array_equal(d["z"][v], np.floor(zf * 16777215.0 + 0.5).astype(np.float32)), (where, mode_setting, wide)


def oracle_project(pcase):
    sh = None
    if pcase["sh_stored"]:
        sh = pcase["sh_u8"].astype(np.float32) if pcase["sh8"] else pcase["sh_sampled"]
    return oracle.project(_oracle_camera(pcase), pcase["centers"], pcase["cov"], pcase["rgba"], sh, scene_indexes=pcase["scene_idx"])


def scene_rejected(pcase):
    """Per splat: does the shader reject its whole scene (sceneOpacity <= 0.01 or not visible, SplatMaterial.js:129-137)?"""
    u = pcase["uniforms"]
    if pcase["build"] != "effects1":
        return np.zeros(pcase["centers"].shape[0], bool)
    gone = np.array([o <= 0.01 or not v for o, v in zip(u["scene_opacity"], u["scene_visibility"])])
    return gone[pcase["scene_idx"]]


def check_dead_blocks(name, pose, pcase, draws, where):
    """(e).  The block counts are asked of the MODE 0 and MODE 1 cells; the accept set of the reference cell, which they all equal."""
    ref = draws[pic.REFERENCE_CELL]
    o = oracle_project(pcase)
    accept = o["visible"] == 1
    assert not (ref["vis"] & ~accept).any(), (where, "the engine draws a splat the oracle's vertex stage rejects")
    centre = np.stack([o["cx"], o["cy"]], axis=1).astype(np.float64)
    b1 = np.stack([o["b1x"], o["b1y"]], axis=1).astype(np.float64)
    b2 = np.stack([o["b2x"], o["b2y"]], axis=1).astype(np.float64)
    check_dropped_splats_miss_the_frame(pcase["uniforms"]["viewport"], centre, b1, b2, accept & ~ref["vis"])
    # a block counts as live by its visible splats - and, where scene effects reject a whole scene (a third of the `effects` case, so no
    # block of it can show 200 visible splats), by the splats of that scene inside the frustum as well: they ran the shader
    counted = scene_rejected(pcase) & pic.frustum_pass(pcase)
    for cell, d in draws.items():
        if d["block_test"] == 2:
            continue
        visible = pic.per_block(d["vis"], d["positions"])
        live = pic.per_block(d["vis"] | counted, d["positions"])
        if pose == "aside":                                     # the box the CPU tier found outside the frustum draws nothing, and
            outside = pic.boxes_outside(pcase, d["positions"])  # blocks beside it do (an eighth of a block: most of what passes the
            assert outside.any() and visible[outside].max() == 0 and visible.max() >= 32, (where, cell, visible.tolist())   # 1.2 w test there lies beyond the frame's edge)
        else:
            assert visible.min() == 0 and live.max() >= 200, (where, cell, visible.tolist(), live.tolist())


def check_strip(ref_full, draws, where):
    """(f): the strip's visible set and rects from the full frame's."""
    r0, r1 = pic.STRIP
    ty0, ty1 = (ref_full["rects"][:, 0] >> 16).astype(np.int64), (ref_full["rects"][:, 1] >> 16).astype(np.int64)
    want = ref_full["vis"] & (ty0 < r1) & (ty1 >= r0)
    assert 50 < want.sum() < ref_full["vis"].sum()
    lo = (ref_full["rects"][:, 0] & 0xFFFF) | (np.clip(ty0, r0, r1 - 1).astype(np.uint32) << 16)
    hi = (ref_full["rects"][:, 1] & 0xFFFF) | (np.clip(ty1, r0, r1 - 1).astype(np.uint32) << 16)
    for cell, d in draws.items():
        assert np.array_equal(d["vis"], want), (where, cell)
        assert np.array_equal(d["rects"][want, 0], lo[want]) and np.array_equal(d["rects"][want, 1], hi[want]), (where, cell)
        assert d["frame"].shape == ((r1 - r0) * pic.TILE, pic.W, 4)


def check_window_depths(name, case, draws):
    """(g), float plane, golden pose: |zrec - (0.5 z + 0.5)| <= 2 dz with z the golden's gl_Position.z of corner 0 (the NDC z: the
    reference shader sets w = 1) and dz the forward error bound of project_instance_cases.window_depth_bound - the golden is an fp32
    evaluation under the same bound, hence twice.  Returns the largest error / bound seen."""
    want = 0.5 * G["vs_" + name][:, 0, 2].astype(np.float64) + 0.5
    _, dz = pic.window_depth_bound(case)
    worst = 0.0
    for cell, d in draws.items():
        if cell[1] == "float":
            v = d["vis"]
            ratio = np.abs(d["z"][v].astype(np.float64) - want[v]) / (2.0 * dz[v])
            worst = max(worst, float(ratio.max()))
    return worst


@pytest.fixture(scope="module")
def base_draws(contexts):
    """The non-EXT base scene of the neutral cases: its reference cell and the two depth cells beside it, per pose and strip."""
    case = pic.make_case(pic.NEUTRAL_BASE)
    out = {}
    for pose, pcase in pic.poses(pic.NEUTRAL_BASE, case).items():
        for rows in (None, pic.STRIP) if pose == "inside" else (None,):
            out[(pose, rows)] = {cell: draw_cell(contexts, pcase, cell, rows) for cell in
                                 (pic.REFERENCE_CELL, ("no_block_cull", "float", True), ("no_block_cull", "unorm24", True))}
    return out


def check_neutral(name, draws, base, where):
    """(d): the EXT kernels on a scene whose EXT uniforms change nothing."""
    for cell, b in base.items():
        d, v = draws[cell], b["vis"]
        if name == "dynamic_identity":                         # view * I in fp32 is exact up to the sign of a zero
            assert np.array_equal(d["vis"], v) and np.array_equal(d["rects"][v], b["rects"][v]), where
            assert np.array_equal(d["recs"][v][:, FLOAT_FIELDS].view(np.float32), b["recs"][v][:, FLOAT_FIELDS].view(np.float32)), where
            assert np.array_equal(d["recs"][v][:, 6:8], b["recs"][v][:, 6:8]), where
            if b["z"] is not None:
                assert np.array_equal(d["z"][v], b["z"][v]), where
        else:
            check_same_draw(d, b, where)
            if b["z"] is not None:
                assert np.array_equal(d["z"].view(np.uint32)[v], b["z"].view(np.uint32)[v]), where


@pytest.mark.parametrize("name", pic.CASES)
def test_every_instance_draws_what_the_golden_and_the_other_instances_draw(contexts, base_draws, name):
    case = pic.make_case(name)
    ref_full = None
    for pose, pcase in pic.poses(name, case).items():
        for rows in (None, pic.STRIP) if pose == "inside" else (None,):
            where = (name, pose, rows)
            draws = {cell: draw_cell(contexts, pcase, cell, rows) for cell in pic.cells(name)}
            check_instances(name, pcase, draws, rows is not None, where)                          # a, c, g
            if pose == "golden" and name in raster_cases.CASES:
                for cell, d in draws.items():                                                     # b
                    check_engine_records(case, G["vs_" + name], d["recs"], d["vis"])
                ratio = check_window_depths(name, case, draws)                                    # g
                print(f"{name}: largest window-depth error / (2 x forward bound) = {ratio:.4f}")
                assert ratio <= 1.0, ratio
            if name in pic.NEUTRAL:
                check_neutral(name, draws, base_draws[(pose, rows)], where)                       # d
            if rows is None and pose != "golden":
                check_dead_blocks(name, pose, pcase, draws, where)                                # e
            if pose == "inside" and rows is None:
                ref_full = draws[pic.REFERENCE_CELL]
            if rows is not None:
                check_strip(ref_full, draws, where)                                               # f
