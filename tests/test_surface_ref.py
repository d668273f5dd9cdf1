"""CPU tier: the host model of the surface pass (surface_ref.py) on fragments whose answer is known by hand, and the measurement
behind its tolerances - the kernel's fp32 expressions restated in np.float32 against fp64 on the scenes the device tests draw."""
import numpy as np
import pytest

import surface_cases as cases
import surface_ref as ref


def synthetic(alphas, power=0.0, w=32, h=32):
    """One list over a 32x32 frame: fragment k covers every pixel with the given power at every pixel (ax = ay = 0 would make the
    power 0; a power p is placed through bx alone at pixel column 0) and alpha alphas[k]."""
    n = len(alphas)
    recs = np.zeros((n, 8), dtype=np.uint32)
    f = np.zeros((n, 6), dtype=np.float32)
    f[:, 0] = -0.5                                           # centre one pixel left of pixel 0's centre: dx = 1 at px = 0
    f[:, 1] = 0.5
    f[:, 2] = np.sqrt(power)                                 # u = ax * dx
    recs[:, :6] = f.view(np.uint32)
    recs[:, 7] = (np.round(np.asarray(alphas) * 65535.0).astype(np.uint32)) << 16
    rects = np.tile(np.array([[0, 1 | (1 << 16)]], dtype=np.uint32), (n, 1))
    return ref.Draw(width=w, height=h, list_shift=1, lists_x=1, list_row_begin=0, ranges=np.array([[0, n]], dtype=np.uint32),
                    entries=np.arange(n, dtype=np.uint32), slots=np.arange(n, dtype=np.uint32), recs=recs, rects=rects,
                    vis=np.ones(n, dtype=bool), z=np.linspace(0.2, 0.8, n))


def answers(draw, tau):
    """Valid answers of pixel (0, 0): (set of entries, whether none is valid)."""
    splats, could, T_lo, T_hi = ref.bin_transmittances(draw, 0, 0, np.array([0]), np.array([0]))
    ok, none_ok = ref.valid_answers(splats, could, T_lo, T_hi, tau)
    return set(np.nonzero(ok[:, 0])[0].tolist()), bool(none_ok[0])


def test_two_stacked_fragments_of_alpha_04_cross_at_the_second():
    assert answers(synthetic([0.4, 0.4]), 0.5) == ({1}, False)
    assert answers(synthetic([0.4, 0.4]), 0.7) == ({0}, False)
    assert answers(synthetic([0.4, 0.4]), 0.3) == (set(), True)


def test_one_fragment_of_alpha_04_does_not_cross():
    assert answers(synthetic([0.4]), 0.5) == (set(), True)


def test_a_fragment_exactly_on_the_cut_is_either():
    on = synthetic([0.9999], power=ref.CUT)                  # a = exp2(-cut) * 1 = 0.0183: crosses tau = 0.99 if it is kept
    assert answers(on, 0.99) == ({0}, True)
    assert answers(synthetic([0.9999], power=ref.CUT - 1e-3), 0.99) == ({0}, False)
    assert answers(synthetic([0.9999], power=ref.CUT + 1e-3), 0.99) == (set(), True)
    # ... and what follows it is judged with and without it: 0.98 x 0.6 crosses 0.59, 1 x 0.6 does not
    both = synthetic([0.9999, 0.4], power=ref.CUT)
    got = ref.bin_transmittances(both, 0, 0, np.array([0]), np.array([0]))
    assert got[2][1, 0] < got[3][1, 0]


def test_check_window_reports_wrong_ids_wrong_depths_and_accepts_right_ones():
    d = synthetic([0.4, 0.4])
    ids = np.full((32, 32), 1, dtype=np.uint32)
    z = np.full((32, 32), d.z[1], dtype=np.float32)
    # only column 0 sees power 0 everywhere?  every pixel does: ax = 0 -> power 0
    assert ref.check_window(d, 0, 0, ids, z, 0.5) == []
    ids[3, 4] = 0
    z[5, 6] = 0.5
    ids[7, 8] = ref.NONE
    bad = ref.check_window(d, 0, 0, ids, z, 0.5)
    assert len(bad) == 3 and "(4, 3)" in bad[0] and "(6, 5)" in bad[1] and "(8, 7)" in bad[2]


def test_fp32_restatement_of_the_power_matches_fp64_on_easy_numbers():
    d = synthetic([0.5], power=2.0)
    p32 = ref.power32(d.recs, 0, 0, np.array([0, 1]), np.array([0, 0]))
    p64 = ref.power64(d.recs, np.array([0, 1]), np.array([0, 0]))
    assert np.allclose(p64[0], [2.0, 8.0], rtol=1e-6) and np.allclose(p32, p64, rtol=1e-6)


@pytest.mark.parametrize("name", ["random5", "random6", "one_opaque", "two_layers", "pile", "occluded", "two_scenes"])
def test_the_tolerances_hold_on_the_test_scenes(name):
    """ETA, DELTA and DEPTH_TOL are 4 x the worst value measured here (surface_ref's docstring records the measurement): the worst
    case of every scene must stay below a quarter of the chosen constant ... within the rounding of the constants themselves."""
    if name.startswith("random"):
        w, h = 150, 90
        from gaussiansplats3d_amd import camera
        cam = camera.demo_camera("garden", w, h)
        scene = cases.random_scene(int(name[6:]))
    else:
        w, h = 64, 64
        cam = cases.small_camera()
        scene = {"one_opaque": cases.one_opaque, "two_layers": cases.two_layers, "occluded": cases.occluded,
                 "pile": lambda c: cases.pile(c, 8), "two_scenes": lambda c: None}[name](cam)
    view = np.asarray(cam.model_view(), np.float64).astype(np.float32)
    proj = np.asarray(cam.projection, np.float64).astype(np.float32)
    if name == "two_scenes":                                # per-scene transforms: only the depth expression differs
        scene, scene_idx, transforms = cases.two_scenes(cam)
        dyn = dict(view_matrix16=np.asarray(cam.view, np.float64).astype(np.float32), transforms=transforms, scene_of_splat=scene_idx)
        eta = eps = 0.0
        vis = np.ones(scene.count, dtype=bool)
    else:
        dyn = {}
        recs, vis = cases.oracle_records(scene, cam, w, h)
        assert vis.any()
        eta, eps = cases.measure_scene(recs, vis, w, h)
    z32 = ref.window_depth(scene.centers[vis], view, proj, dtype=np.float32, **dyn)
    z64 = ref.window_depth(scene.centers[vis], view, proj, dtype=np.float64, **dyn)
    assert np.isfinite(z64).all() and (z64 > 0).all() and (z64 < 1).all()
    zerr = float(np.abs(z32.astype(np.float64) - z64).max())
    print(f"{name}: worst |power32 - power64| = {eta:.3e}, worst relative alpha error = {eps:.3e}, worst depth error = {zerr:.3e}")
    assert 4.0 * eta <= ref.ETA and 4.0 * eps <= ref.DELTA and 4.0 * zerr <= ref.DEPTH_TOL
