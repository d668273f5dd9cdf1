"""-m gpu: the HIP vertex stage on the DESIGNED edge cases (tests/raster_edge_cases.py), held to what the reference's own GLSL computed
for them (tests/golden/raster_edge_ref.npz; only the .npz is read).  Every drawn splat of these cases is large and inside enough that
the engine's thin-or-outside drop cannot apply (the CPU tier asserts it on the shader's outputs), so no band applies to a verdict:
  verdicts   on_screen == drawn on every splat - half of each knife-edge sub-case by the last bit of the discriminant, every ladder at
             the float the shader changes at - and the records pass test_raster_ref.check_engine_records unchanged;
  instances  every k_project instance a case can reach (tests/project_instance_cases.py: MODE 0 / 1 / 2, no destination and the two
             destination depth formats over a far plane, both look-up words) launches as planned, draws the shader's verdicts and
             equals the reference cell bit for bit in mask, slots, rects, records and frame; a case that is not EXT equals its twin
             with three unused scene indexes, which runs the EXT kernels;
  strips     two-row strips tile the full frame's verdicts, rects and pixels (the knife-edge splats are drawn TALL although their
             covariance is wide: the strip pre-test must bound them by max(a, d));
  frames     one sorted frame per camera kind of the knife-edge class within helpers.compare_frames' gates of oracle.render."""
import os

import numpy as np
import pytest

import helpers
import oracle
import project_instance_cases as pic
import raster_edge_cases as rec
import raster_edge_ref
import test_gpu_project_instances as instances
from gaussiansplats3d_amd import Context, SplatMesh
from oracle.make_golden_raster import shader_verdicts
from test_gpu_permutations import _order, _strips_equal_frame
from test_gpu_project_instances import check_same_draw, contexts, draw_cell, narrow_of   # noqa: F401 (contexts: a fixture)
from test_raster_ref import _oracle_camera, check_engine_records, engine_mesh

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_edge_ref.npz"))
STRIP_CASES = rec.KNIFE_CASES + ["knife_points", "planes_persp", "planes_ortho", "scene_ladders", "arith_ortho", "arith_aa", "cap_1024", "cap_48",
                                 "fade_ladders", "clip_block"]


@pytest.fixture(scope="module")
def golden():
    """name -> (case, the shader's outputs, the shader's verdicts): built on first use."""
    made = {}

    def get(name):
        if name not in made:
            res = rec.unpack(G["vs_" + name])
            made[name] = (rec.make_case(name), res, shader_verdicts(res)[0])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def edge_mesh(ctx, case):
    """engine_mesh - and for the two cases it cannot express (storage in upload order, half covariances given as bits because
    toHalfFloat would clamp an inf away) the same mesh built here; neither case has scenes or a fade."""
    if not (case.get("keep_order") or case.get("half_bits")):
        return engine_mesh(ctx, case)
    u, sc = case["uniforms"], case["scene"]
    assert case["scene_idx"] is None and u["fade_in_complete"] and not case["sh8"]
    mesh = SplatMesh(ctx, sc.count, sc.sh_degree, half_precision_covariances=case["cov_half"], antialiased=case["antialiased"],
                     kernel_2d_size=case["kernel2d"], max_screen_space_splat_size=case["max_splat_px"], splat_scale=u["splat_scale"],
                     point_cloud_mode=bool(u["point_cloud"]), keep_order=bool(case.get("keep_order")))
    sh = sc.sh if sc.sh_degree else None
    if case.get("half_bits"):
        mesh.build(sc.centers, case["cov16"], sc.rgba, sh, covariances_are_half_bits=True)
    else:
        mesh.build(sc.centers, sc.cov, sc.rgba, sh)
    mesh.set_camera(case["camera"], focal_adjustment=1.0 / u["inverse_focal_adjustment"], spherical_harmonics_degree=u["sh_degree"])
    return mesh


@pytest.fixture(scope="module", autouse=True)
def cells_build_edge_meshes():
    """test_gpu_project_instances.draw_cell builds its mesh with that module's engine_mesh: the edge cases' builder for this module."""
    mp = pytest.MonkeyPatch()
    mp.setattr(instances, "engine_mesh", edge_mesh)
    yield
    mp.undo()


def in_upload_order(mesh, case):
    n = case["scene"].count
    mesh.update_render_indexes(np.arange(n, dtype=np.uint32), n)


def say_where(case, wrong):
    """The groups of the splats in `wrong`, for a failure's message."""
    return {group: np.intersect1d(g["idx"], wrong)[:8].tolist() for group, g in case["groups"].items() if np.isin(g["idx"], wrong).any()}


@pytest.mark.parametrize("name", rec.CASES)
def test_the_engine_draws_exactly_what_the_shader_draws(ctx, golden, name):
    case, res, drawn = golden(name)
    mesh = edge_mesh(ctx, case)
    try:
        in_upload_order(mesh, case)
        mesh.render()
        recs, rects, on_screen = mesh.debug_records()
        wrong = np.flatnonzero(on_screen != drawn)
        print(f"{name}: the shader draws {int(drawn.sum())} of {len(drawn)}, the engine {int(on_screen.sum())}")
        assert len(wrong) == 0, (name, len(wrong), say_where(case, wrong))
        check_engine_records(case, res, recs, on_screen)
        if name in ("cap_1024", "cap_48"):                    # the footprint stops growing at the float the restatement names
            capped = raster_edge_ref.verdicts(case, capped=True)[0]
            for ladder in case["groups"]["cap"]["ladders"]:
                axes = recs[ladder][:, 2:4]                   # SplatRec ax, ay: K * basisVector1 / |basisVector1|^2
                same = (axes == axes[-1]).all(axis=1)
                assert same[capped[ladder]].all() and not same[:2].any(), (name, same.tolist())
    finally:
        mesh.dispose()


@pytest.mark.parametrize("name", rec.CASES)
def test_every_instance_draws_the_shaders_verdicts_bit_for_bit(contexts, golden, name):
    case, res, drawn = golden(name)
    cells = pic.cells("dynamic" if case["dynamic"] else "sh0")
    draws = {cell: draw_cell(contexts, case, cell) for cell in cells}
    ref = draws[pic.REFERENCE_CELL]
    for cell, d in draws.items():
        planned = pic.planned_instance(case, cell, False, narrow_of)
        ran = (d["instance"] & 1, d["block_test"], (d["instance"] >> 1) & 1, (d["instance"] >> 2) & 1)
        assert ran == planned, (name, cell, "planned", planned, "ran", ran)
        wrong = np.flatnonzero(d["vis"] != drawn)
        assert len(wrong) == 0, (name, cell, len(wrong), say_where(case, wrong))
        check_same_draw(d, ref, (name, cell))
    assert {(p[1], p[2], p[3]) for p in (pic.planned_instance(case, c, False, narrow_of) for c in cells)} == \
        {(m, d, w) for m in ((2,) if case["dynamic"] else (0, 1, 2)) for d in (0, 1) for w in (0, 1)}
    if name in rec.NEUTRAL_TWINS:                             # the EXT kernels with nothing for them to do
        twin = rec.neutral_twin(case)
        assert not pic.ext_rule(case) and pic.ext_rule(twin)
        for cell in cells:
            d = draw_cell(contexts, twin, cell)
            assert d["instance"] & 1, (name, cell)
            check_same_draw(d, ref, (name, "twin", cell))


@pytest.mark.parametrize("name", STRIP_CASES)
def test_two_row_strips_tile_the_frames_verdicts(ctx, golden, name):
    case, res, drawn = golden(name)
    mesh = edge_mesh(ctx, case)
    try:
        in_upload_order(mesh, case)
        mesh.render()
        _, rects, full = mesh.debug_records()
        assert np.array_equal(full, drawn), name
        ty0, ty1 = (rects[:, 0] >> 16).astype(np.int64), (rects[:, 1] >> 16).astype(np.int64)
        rows = (rec.H + 15) // 16
        several = 0
        for r0 in range(0, rows, 2):
            r1 = min(r0 + 2, rows)
            mesh.render(tile_rows=(r0, r1))
            _, srects, vis = mesh.debug_records()
            want = full & (ty0 < r1) & (ty1 >= r0)
            wrong = np.flatnonzero(vis != want)
            assert len(wrong) == 0, (name, (r0, r1), len(wrong), say_where(case, wrong))
            lo = (rects[:, 0] & 0xFFFF) | (np.clip(ty0, r0, r1 - 1).astype(np.uint32) << 16)
            hi = (rects[:, 1] & 0xFFFF) | (np.clip(ty1, r0, r1 - 1).astype(np.uint32) << 16)
            assert np.array_equal(srects[want, 0], lo[want]) and np.array_equal(srects[want, 1], hi[want]), (name, (r0, r1))
            several += int(want.sum())
        if name in rec.KNIFE_CASES:                           # the splats are large: on average each reaches more than two strips
            assert several > 2 * int(full.sum())
        _strips_equal_frame(mesh, case["camera"], name)
    finally:
        mesh.dispose()


@pytest.mark.parametrize("kind", list(rec.CAMERA_KINDS))
def test_sorted_frame_of_the_knife_edge_class_matches_the_raster_oracle(ctx, golden, kind):
    name = rec.CAMERA_KINDS[kind]
    case, res, drawn = golden(name)
    mesh = edge_mesh(ctx, case)
    try:
        order = _order(case["scene"], case["camera"])
        mesh.update_render_indexes(order, case["scene"].count)
        got, _ = mesh.render()
        fb, q, amb, frags = oracle.render(_oracle_camera(case), case["centers"], case["cov"], case["rgba"], case["sh_sampled"], order,
                                          scene_indexes=case["scene_idx"])
        assert frags > 1000
        print(helpers.compare_frames(got, fb, amb, name))
    finally:
        mesh.dispose()
