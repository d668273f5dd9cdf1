"""Seeded inputs of the COMBINED shader permutations: a second case list beside tests/raster_cases.py, for the cases in which several
features of the vertex stage are on together (per-scene 8-bit SH ranges, scene indexes without dynamicMode or effects, dynamicMode +
enableOptionalEffects + antialiased + fade-in, dynamic + orthographic, the size clamp under a per-scene transform, all 32 scenes).
oracle/make_golden_raster.py --combos pushes them through the reference's own shader text into tests/golden/raster_combo_ref.npz;
tests/test_raster_combo_ref.py holds the C raster oracle to it and tests/test_gpu_raster_combos.py the HIP vertex stage.

A case is what raster_cases.make_case builds, with two differences: uniforms["sh8_range"] is a LIST, one (min, max) per scene, and the
case says itself which shader #defines are on (case["dynamic"], case["effects"]) - a build name such as "dyn_fx_aa2" is not parsed."""
import numpy as np

import helpers
import raster_cases
from gaussiansplats3d_amd import camera
from gaussiansplats3d_amd.util import to_half_three

GS_MAX_SCENES = 32
N, W, H = 2000, 512, 288
FADE_DISTANCE = 0.75                                          # SplatMaterial.js:354


def shader_builds():
    """The builds the combo cases run through: three of raster_cases.shader_builds() and three new ones."""
    old = raster_cases.shader_builds()
    base = {k: v for k, v in old["base2"].items() if k != "maxSphericalHarmonicsDegree"}
    return {
        "base2": old["base2"], "dynamic2": old["dynamic2"], "effects1": old["effects1"],
        "dyn_fx_aa2": dict(base, maxSphericalHarmonicsDegree=2, dynamicMode=True, enableOptionalEffects=True, antialiased=True),
        "dyn_fx_small1": dict(base, maxSphericalHarmonicsDegree=1, dynamicMode=True, enableOptionalEffects=True,
                              maxScreenSpaceSplatSize=48, kernel2DSize=0.1),
        "fx_aa2": dict(base, maxSphericalHarmonicsDegree=2, enableOptionalEffects=True, antialiased=True),
    }


def census_builds():
    """The antialiased builds without `antialiased`: run only while the golden is made, to count the splats that the antialiased
    `alpha < 1/255` rule ALONE rejects (rejected by the antialiased build, drawn by its sibling).  No output of theirs is stored."""
    b = shader_builds()
    return {"dyn_fx2": dict(b["dyn_fx_aa2"], antialiased=False), "fx2": dict(b["fx_aa2"], antialiased=False)}


CENSUS_SIBLING = {"dyn_fx_aa2": "dyn_fx2", "fx_aa2": "fx2"}

CASES = ["scenes_sh8", "dyn_fx_aa_sh8_fade", "dyn_ortho_aa", "dyn_fx_clamp", "fx_ortho_points_fade", "fx_aa_fade_eval1",
         "dyn_fx_32_scenes"]
FADE_CASES = ["dyn_fx_aa_sh8_fade", "fx_ortho_points_fade", "fx_aa_fade_eval1"]
AA_REJECT_CASES = ["fx_aa_fade_eval1", "dyn_fx_aa_sh8_fade"]


def _garden():
    up, pos, look = (np.asarray(v, np.float64) for v in camera.DEMO_POSES["garden"])
    fwd = (look - pos) / np.linalg.norm(look - pos)
    return up, pos, look, fwd


def _about(point, m3, shift=(0.0, 0.0, 0.0)):
    """Column-major elements of the 4 x 4 that applies the 3 x 3 `m3` about `point`, then moves by `shift`."""
    t = np.eye(4)
    t[:3, :3] = m3
    t[:3, 3] = point - m3 @ point + np.asarray(shift)
    return t.T.reshape(16)


def _turn(axis, angle):
    """Rotation by `angle` about the unit vector `axis` (Rodrigues)."""
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _rot_y(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]], [0, 0, 0, 1]]).T.reshape(16)


IDENTITY = np.eye(4).T.reshape(16)


def _fade(sc):
    """(sceneCenter, visibleRegionFadeStartRadius): about half of the splats inside the start radius."""
    center = sc.centers.mean(axis=0)
    return center.astype(np.float32).tolist(), float(np.median(np.linalg.norm(sc.centers - center, axis=1)))


def make_case(name):
    up, pos, look, fwd = _garden()
    cam = camera.demo_camera("garden", W, H)
    slab = pos + fwd * 4.65                                    # the middle of helpers.small_scene's slab
    n = N
    case = dict(cov_half=False, sh8=False, scene_idx=None, kernel2d=0.3, max_splat_px=1024.0, antialiased=False, dynamic=False,
                effects=False)
    _u = raster_cases._uniforms

    def every(k):
        return (np.arange(n) % k).astype(np.uint32)

    if name == "scenes_sh8":                      # scene_count > 1 alone switches the scene index read on; the ranges need it
        sc = helpers.small_scene(n, 2, seed=401, cov_half=True)
        case.update(build="base2", cov_half=True, sh8=True, scene_idx=every(4),
                    uniforms=_u(cam, 2, scene_count=4, sh8_range=[(-1.5, 1.5), (-0.9, 1.1), (-0.6, 0.7), (-2.0, 1.2)]))
    elif name == "dyn_fx_aa_sh8_fade":            # the reference's `dynamicScene: true` with several level-2 .ksplat scenes
        sc = helpers.small_scene(n, 2, seed=402, scale=0.006, cov_half=True)
        transforms = [_rot_y(0.3, (0.4, -0.2, 0.1)),                               # a rotation + translation
                      _about(slab, np.diag([1.3, -0.8, 0.7])),                     # non-uniform, one axis mirrored
                      IDENTITY,                                                    # (below the opacity cut)
                      _about(pos, _turn(fwd, np.pi / 2)),                          # a quarter turn about the view axis
                      IDENTITY]                                                    # (invisible)
        case.update(build="dyn_fx_aa2", cov_half=True, sh8=True, antialiased=True, dynamic=True, effects=True, scene_idx=every(5),
                    uniforms=_u(cam, 2, scene_count=5, transforms=transforms, opacity=[1.0, 0.4, 0.005, 0.7, 1.0],
                                visible=[1, 1, 1, 1, 0], fade=_fade(sc),
                                sh8_range=[(-1.5, 1.5), (-0.9, 1.1), (-0.7, 0.8), (-0.6, 0.7), (-2.0, 1.2)]))
    elif name == "dyn_ortho_aa":                  # the per-scene model-view feeds the orthographic J
        sc = helpers.small_scene(n, 2, seed=403)
        cam = camera.OrthographicCamera(W, H, pos, look, up, zoom=40.0)
        big = np.diag([1.2, 1.2, 1.2, 1.0]); big[:3, 3] = (-0.5, 0.3, 0.0)
        transforms = [IDENTITY, _rot_y(0.3, (0.4, -0.2, 0.1)), big.T.reshape(16)]
        case.update(build="dyn_fx_aa2", antialiased=True, dynamic=True, effects=True, scene_idx=every(3),
                    uniforms=_u(cam, 2, scene_count=3, transforms=transforms, opacity=[1.0, 1.0, 1.0], visible=[1, 1, 1],
                                splat_scale=1.7))
    elif name == "dyn_fx_clamp":                  # the 48-px clamp under a per-scene transform that scales by 1.6
        sc = helpers.small_scene(n, 1, seed=404, scale=0.2)
        big = np.diag([1.6, 1.6, 1.6, 1.0]); big[:3, 3] = slab - 1.6 * slab
        transforms = [IDENTITY, big.T.reshape(16), _rot_y(-0.2, (0.1, 0.2, -0.3))]
        case.update(build="dyn_fx_small1", sh8=True, kernel2d=0.1, max_splat_px=48.0, dynamic=True, effects=True, scene_idx=every(3),
                    uniforms=_u(cam, 1, scene_count=3, transforms=transforms, opacity=[1.0, 0.6, 0.9], visible=[1, 1, 1],
                                splat_scale=1.7, focal_adjustment=2.0, sh8_range=[(-1.5, 1.5), (-0.8, 0.9), (-1.1, 0.6)]))
    elif name == "fx_ortho_points_fade":
        sc = helpers.small_scene(n, 1, seed=405)
        cam = camera.OrthographicCamera(W, H, pos, look, up, zoom=40.0)
        case.update(build="effects1", effects=True, scene_idx=every(3),
                    uniforms=_u(cam, 1, scene_count=3, opacity=[1.0, 0.4, 0.005], visible=[1, 1, 1], point_cloud=True, fade=_fade(sc)))
    elif name == "fx_aa_fade_eval1":              # the antialiased reject, then scene opacity, then the fade: the order of the product
        sc = helpers.small_scene(n, 2, seed=406, scale=0.006)
        case.update(build="fx_aa2", sh8=True, antialiased=True, effects=True, scene_idx=every(3),
                    uniforms=_u(cam, 2, sh_degree=1, scene_count=3, opacity=[1.0, 0.5, 0.8], visible=[1, 1, 1], fade=_fade(sc),
                                sh8_range=[(-1.5, 1.5), (-0.9, 1.1), (-0.6, 0.7)]))
    elif name == "dyn_fx_32_scenes":              # the end of every per-scene table
        sc = helpers.small_scene(n, 2, seed=407)
        rng = np.random.default_rng(4070)
        k = GS_MAX_SCENES
        transforms = [_about(slab, _turn(fwd, a) * s_, d) for a, s_, d in
                      zip(rng.uniform(-0.4, 0.4, k), rng.uniform(0.8, 1.25, k), rng.uniform(-0.3, 0.3, (k, 3)))]
        lo, hi = rng.uniform(-2.0, -0.5, k), rng.uniform(0.5, 2.0, k)
        case.update(build="dyn_fx_aa2", sh8=True, antialiased=True, dynamic=True, effects=True, scene_idx=every(k),
                    uniforms=_u(cam, 2, scene_count=k, transforms=transforms, opacity=rng.uniform(0.05, 1.0, k).tolist(),
                                visible=[1] * k, sh8_range=list(zip(lo.tolist(), hi.tolist()))))
    else:
        raise KeyError(name)
    u = case["uniforms"]
    if not isinstance(u["sh8_range"], list):
        u["sh8_range"] = [u["sh8_range"]] * max(u["scene_count"], 1)
    cov = sc.cov
    case["cov16"] = to_half_three(cov) if case["cov_half"] else None
    if case["cov_half"]:
        cov = case["cov16"].view(np.float16).astype(np.float32)
    sh = sc.sh.astype(np.float32) if sc.sh_degree else np.zeros((n, 0), np.float32)      # fp16 storage, widened by the sampler
    sh_u8 = None
    if case["sh8"]:                               # compression level 2: uint8 storage by the splat's own scene's range
        of = case["scene_idx"] if case["scene_idx"] is not None else np.zeros(n, np.uint32)
        lo = np.array([r[0] for r in u["sh8_range"]], np.float32)[of][:, None]
        hi = np.array([r[1] for r in u["sh8_range"]], np.float32)[of][:, None]
        sh_u8 = np.clip(np.floor((np.clip(sh, lo, hi) - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)
        sh = sh_u8.astype(np.float32) / np.float32(255.0)
    case.update(scene=sc, camera=cam, centers=sc.centers, cov=cov, rgba=sc.rgba, sh_stored=sc.sh_degree, sh_sampled=sh, sh_u8=sh_u8)
    return case


def scene_rejected(case):
    """Per scene: does the shader reject it whole (sceneOpacity <= 0.01 or not visible, SplatMaterial.js:129-137)?"""
    u = case["uniforms"]
    k = max(u["scene_count"], 1)
    if not case["effects"]:
        return np.zeros(k, bool)
    return np.array([o <= 0.01 or not v for o, v in zip(u["scene_opacity"], u["scene_visibility"])])


def fade_factor(case):
    """distanceLoadFadeInFactor of SplatMaterial.js:347-363 per splat in fp64 (1 where the fade-in is complete)."""
    u = case["uniforms"]
    if u["fade_in_complete"]:
        return np.ones(case["centers"].shape[0])
    d = np.linalg.norm(case["centers"].astype(np.float64) - np.asarray(u["scene_center"], np.float64), axis=1)
    return np.where(d < u["fade_start_radius"], 1.0, 1.0 - np.clip((d - u["fade_start_radius"]) / FADE_DISTANCE, 0.0, 1.0))
