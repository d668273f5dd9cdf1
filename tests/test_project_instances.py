"""CPU tier of the vertex stage's instance matrix (tests/project_instance_cases.py): the planned cells reach all 24 k_project
instances, by the host models of the launch rule - draw_plan_ref.block_test_mode, the library's own narrow_bin_word through its
pure-host entry (tests/test_bin_word.py) and gs_launch_project's `ext` rule - and the poses the GPU tier counts on for dead storage
blocks really have them, in float64.  No device."""
import itertools

import numpy as np
import pytest

import project_instance_cases as pic
import raster_cases
import strip_cull_cases
from test_bin_word import word

ALL_INSTANCES = set(itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1)))          # (EXT, MODE, DEPTH, NARROW)
EXT_CASES = {"orthographic", "fade_in", "sh8", "effects", "dynamic", "effects_neutral", "scenes_neutral", "dynamic_identity"}


def narrow_of(tiles_x, tiles_y, switch):
    return word(tiles=(tiles_x, tiles_y), switch=switch).narrow


def planned(name, case, strip=False):
    return {pic.planned_instance(case, cell, strip, narrow_of) for cell in pic.cells(name)}


@pytest.fixture(scope="module")
def cases():
    return {name: pic.make_case(name) for name in pic.CASES + [pic.NEUTRAL_BASE]}


def test_the_planned_cells_reach_all_24_instances(cases):
    assert len(ALL_INSTANCES) == 24
    reached = set()
    for name in pic.CASES:
        for strip in (False, True):
            got = planned(name, cases[name], strip)
            # what each case contributes: its EXT column, every MODE the block cull allows, with and without window depths, both words
            ext = int(name in EXT_CASES)
            modes = (2,) if name in pic.DYNAMIC else (0, 1, 2)
            assert got == set(itertools.product((ext,), modes, (0, 1), (0, 1))), (name, strip, sorted(got))
            reached |= got
    assert reached == ALL_INSTANCES, sorted(ALL_INSTANCES - reached)
    # the golden rows alone reach them too: the neutral cases add observers, not instances
    assert set().union(*(planned(n, cases[n]) for n in raster_cases.CASES)) == ALL_INSTANCES


def test_every_instance_is_reached_by_a_case_with_a_golden_and_by_a_strip(cases):
    for strip in (False, True):
        by_instance = {}
        for name in raster_cases.CASES:
            for inst in planned(name, cases[name], strip):
                by_instance.setdefault(inst, []).append(name)
        assert set(by_instance) == ALL_INSTANCES
        for inst, names in by_instance.items():
            assert len(names) >= 4, (inst, names)              # (EXT kernels with a block test: orthographic, fade_in, sh8, effects)


def test_the_base_of_the_neutral_cases_is_not_ext_and_shares_their_scene(cases):
    base = cases[pic.NEUTRAL_BASE]
    assert not pic.ext_rule(base) and base["scene_idx"] is None
    for name in pic.NEUTRAL:
        c = cases[name]
        assert pic.ext_rule(c)
        for key in ("centers", "cov", "rgba", "sh_sampled"):
            assert np.array_equal(c[key], base[key])
        assert c["uniforms"]["model_view"].tolist() == base["uniforms"]["model_view"].tolist()
    assert cases["effects_neutral"]["uniforms"]["scene_opacity"] == [1.0, 1.0, 1.0]
    assert all(np.array_equal(t, np.eye(4).reshape(16)) for t in cases["dynamic_identity"]["uniforms"]["transforms"])


@pytest.mark.parametrize("name", [n for n in pic.CASES + [pic.NEUTRAL_BASE] if n not in pic.DYNAMIC])
def test_the_inside_pose_has_dead_and_live_storage_blocks(cases, name):
    """At least one 256-splat storage block without a single splat that passes the frustum rejects and at least one with 200 or more
    (eight blocks of Morton order, host restatement): what the MODE 0 and MODE 1 cells of the GPU tier must drop and must keep."""
    case = cases[name]
    n = case["centers"].shape[0]
    positions = strip_cull_cases.morton_positions(case["centers"], [(0, n)])
    live = pic.per_block(pic.frustum_pass(pic.poses(name, case)["inside"]), positions)
    print(name, live.tolist())
    assert live.shape[0] == 8 and live.min() == 0 and live.max() >= 200, live.tolist()
    golden = pic.per_block(pic.frustum_pass(case), positions)
    assert golden.min() > 0, golden.tolist()                   # (the golden pose has no dead block: the gap the inside pose closes)


def test_the_orthographic_aside_pose_puts_a_whole_block_box_outside(cases):
    """No eye on the viewing axis can (project_instance_cases.ASIDE_RIGHT says why); from the side, one block's box fails x > 1.2 w at
    every corner by ten times the block test's tolerance, and other blocks are mostly in view."""
    case = cases["orthographic"]
    positions = strip_cull_cases.morton_positions(case["centers"], [(0, case["centers"].shape[0])])
    all_poses = pic.poses("orthographic", case)
    assert not pic.boxes_outside(all_poses["inside"], positions).any()
    aside = all_poses["aside"]
    outside = pic.boxes_outside(aside, positions)
    live = pic.per_block(pic.frustum_pass(aside), positions)
    print(outside.tolist(), live.tolist())
    assert outside.any() and live[outside].max() == 0 and live.max() >= 128


def test_window_depth_bound_is_finite_where_it_is_used(cases):
    for name in raster_cases.CASES:
        case = cases[name]
        z, dz = pic.window_depth_bound(case)
        keep = pic.frustum_pass(case)
        assert keep.sum() > 100 and np.isfinite(z[keep]).all() and np.isfinite(dz[keep]).all() and (dz[keep] > 2.0 ** -24).all()
        assert np.median(dz[keep]) < 1e-5                      # (a few ulps of a depth near 1: the bound is no blanket tolerance)
