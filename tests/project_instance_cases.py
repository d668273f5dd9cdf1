"""The vertex stage's instance matrix: k_project (csrc/project.hip) is compiled once per (EXT, MODE, DEPTH, NARROW) - 24 kernels,
each with its own register allocation - and this module says which scenes, switches and destinations make a draw launch each of
them.  No device is needed here: tests/test_project_instances.py holds the plan to the host models of the launch rule (all 24
tuples must be planned), tests/test_gpu_project_instances.py draws every cell and holds it to the shader goldens.

  rows     the twelve raster_cases.CASES (each has a golden of the reference's shader) and three EXT scenes that must draw exactly
           what their non-EXT base scene draws: scene effects at opacity 1, three scene indexes with nothing else, per-scene
           transforms that are all the identity
  MODE     the switch a mesh is created under: none (a fresh mesh has measured nothing: 1), $GSPLAT_NO_BLOCK_LIST (0),
           $GSPLAT_NO_BLOCK_CULL (2).  Every draw of the GPU tier is the first draw of a fresh mesh, so the measured share of the
           scene in view never moves a cell to another mode.  Per-scene transforms switch the block cull off: MODE 2 whatever is set
  DEPTH    no destination / a float32 depth plane of 1.0 (nothing is occluded) / the same plane as 24-bit fixed point
  NARROW   $GSPLAT_NO_COMPACT_BIN_WORD around the draw selects the 8-byte look-up word
  poses    the case's own camera (the golden pose: every storage block has live splats there) and one INSIDE the cloud, where two to
           three of the eight storage blocks hold no splat that passes the frustum rejects; the orthographic case, whose block test
           cannot see a dead block from any eye on the viewing axis, also from beside its frustum (ASIDE_RIGHT below)
  strip    tile rows 5 .. 10 at the inside pose
Whoever adds a template axis to k_project adds it here: test_project_instances.py fails until the plan covers the new instances."""
import numpy as np

import draw_plan_ref
import raster_cases
from gaussiansplats3d_amd import camera

NEUTRAL_BASE = "neutral_base"                                  # the non-EXT scene the three neutral cases are compared with
NEUTRAL = ["effects_neutral", "scenes_neutral", "dynamic_identity"]
CASES = list(raster_cases.CASES) + NEUTRAL
DYNAMIC = ("dynamic", "dynamic_identity")                      # pp.block_cull == 0: MODE 2 only

MODE_SWITCH = {"default": None, "no_block_list": "GSPLAT_NO_BLOCK_LIST", "no_block_cull": "GSPLAT_NO_BLOCK_CULL"}
DEPTHS = ("none", "float", "unorm24")
WIDE_SWITCH = "GSPLAT_NO_COMPACT_BIN_WORD"
REFERENCE_CELL = ("no_block_cull", "none", True)               # MODE 2, no destination, the 8-byte word: no block test at all
INSIDE_ADVANCE = 4.5                                           # the inside pose: eye = garden eye + 4.5 x forward ...
# ... moved along forward for the seeds whose fullest block holds too few splats in the frustum at 4.5 (the dead-block precondition
# of test_project_instances.py asks for 200, and the GPU tier for 200 that DRAW - a few of those in the frustum are too thin to
# reach a pixel centre, and the 1.2 w test passes splats up to a fifth of the frame beyond its edges, which 1.3-px points do not
# reach back from): sh2 has 187 at 4.5 and 208 at 4.0, point_cloud 190 and 228 at 3.0, fade_in 202 and 208 at 4.25
INSIDE_ADVANCE_OF = {"sh2": 4.0, "point_cloud": 3.0, "fade_in": 4.25}
# Under the orthographic projection w = 1 and the z reject of the 1.2 w test lies 100 units behind the eye, so no eye on the viewing
# axis puts a block outside it: the blocks behind the inside pose go by GL's clip of ndc.z, per splat, and the block test keeps them.
# The orthographic case therefore has a third pose, the golden eye moved 8.5 to its right with the same direction and zoom: the box
# of one storage block lies beyond x > 1.2 w (the block test must drop it) next to blocks that are mostly inside the 1.2 w frustum
# (162 of 256 at most; the cloud is narrower than the frustum, so most of those lie in its margin beyond the frame and few draw).
ASIDE_RIGHT = 8.5
STRIP = (5, 11)
W, H, TILE = 512, 288, 16


def make_case(name):
    """raster_cases.make_case for its twelve names; the neutral cases and their base share the scene of seed 311 at SH degree 1."""
    if name in raster_cases.CASES:
        return raster_cases.make_case(name)
    case = raster_cases.make_case("effects")                   # small_scene(2000, 1, seed=311), the garden camera
    n = case["scene"].count
    three = (np.arange(n) % 3).astype(np.uint32)
    cam = case["camera"]
    if name == NEUTRAL_BASE:
        case.update(build="base1", scene_idx=None, uniforms=raster_cases._uniforms(cam, 1))
    elif name == "effects_neutral":
        case.update(build="effects1", scene_idx=three,
                    uniforms=raster_cases._uniforms(cam, 1, scene_count=3, opacity=[1.0, 1.0, 1.0], visible=[1, 1, 1]))
    elif name == "scenes_neutral":                             # EXT through scene_count > 1 alone
        case.update(build="base1", scene_idx=three, uniforms=raster_cases._uniforms(cam, 1, scene_count=3))
    elif name == "dynamic_identity":                           # ("dynamic2" names the dynamicMode build; the scene stays SH degree 1)
        case.update(build="dynamic2", scene_idx=three,
                    uniforms=raster_cases._uniforms(cam, 1, scene_count=3, transforms=[np.eye(4).T.reshape(16)] * 3))
    else:
        raise KeyError(name)
    return case


def moved_camera(case, advance=0.0, right=0.0):
    """The garden camera moved `advance` along its viewing direction and `right` along its x axis, looking the same way: same size,
    up vector and zoom."""
    up, pos, look = (np.asarray(v, dtype=np.float64) for v in camera.DEMO_POSES["garden"])
    fwd = (look - pos) / np.linalg.norm(look - pos)
    cam = case["camera"]
    eye = pos + advance * fwd + right * np.asarray(cam.matrix_world, np.float64)[0:3]
    if getattr(cam, "is_orthographic", False):
        return camera.OrthographicCamera(cam.width, cam.height, tuple(eye), tuple(eye + fwd), tuple(up), zoom=cam.zoom)
    return camera.PerspectiveCamera(cam.width, cam.height, tuple(eye), tuple(eye + fwd), tuple(up))


def with_camera(case, cam):
    """The case seen by another camera of the same size and kind: the camera-derived uniforms follow, everything else stays."""
    out = dict(case)
    u = dict(case["uniforms"])
    fa = 1.0 / u["inverse_focal_adjustment"]
    u.update(model_view=cam.model_view(), projection=cam.projection, view_matrix=cam.view, camera_position=cam.position,
             focal=cam.focal(fa))
    assert (cam.width, cam.height) == tuple(u["viewport"])
    out.update(uniforms=u, camera=cam)
    return out


def poses(name, case):
    """{pose name: the case as that pose sees it}: golden (the case's own camera), inside, and aside for the orthographic case."""
    out = {"golden": case, "inside": with_camera(case, moved_camera(case, advance=INSIDE_ADVANCE_OF.get(name, INSIDE_ADVANCE)))}
    if name == "orthographic":
        out["aside"] = with_camera(case, moved_camera(case, right=ASIDE_RIGHT))
    return out


# -- which instance a cell launches: host models of gs_launch_project's rule ----------------------------------------------------
def ext_rule(case):
    """gs_launch_project's `ext`: 8-bit SH, more than one scene, or an orthographic / fade-in / scene-effects / dynamic camera flag."""
    u = case["uniforms"]
    several = case["scene_idx"] is not None and u["scene_count"] > 1
    return bool(case["sh8"] or several or u["orthographic"] or not u["fade_in_complete"] or case["build"] in ("effects1", "dynamic2"))


def planned_mode(case, mode_setting, strip):
    """draw_plan.cpp's block_test_mode for the first draw of a mesh created under the setting's switch (nothing measured yet)."""
    block_cull = case["build"] != "dynamic2" and mode_setting != "no_block_cull"
    return draw_plan_ref.block_test_mode(0, 0, strip, block_cull, mode_setting == "no_block_list", False)


def cells(name):
    """The (mode setting, depth setting, wide switch set) cells a case draws."""
    settings = ["no_block_cull"] if name in DYNAMIC else list(MODE_SWITCH)
    return [(m, d, w) for m in settings for d in DEPTHS for w in (True, False)]


def planned_instance(case, cell, strip, narrow_of):
    """(EXT, MODE, DEPTH, NARROW) of a cell's draw.  narrow_of(tiles_x, tiles_y, switch) is draw_plan.cpp's narrow_bin_word, which the
    caller reads from the library's pure-host entry (tests/test_bin_word.py)."""
    mode_setting, depth, wide = cell
    tiles = ((W + TILE - 1) // TILE, (H + TILE - 1) // TILE)
    return (int(ext_rule(case)), planned_mode(case, mode_setting, strip), int(depth != "none"), int(narrow_of(*tiles, int(wide))))


# -- the dead-block precondition (float64, no device) ---------------------------------------------------------------------------
def clip_coordinates(case, points):
    u = case["uniforms"]
    mv = np.asarray(u["model_view"], np.float64).reshape(4, 4).T
    p = np.asarray(u["projection"], np.float64).reshape(4, 4).T
    pts = np.asarray(points, np.float64)
    return np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1) @ (p @ mv).T


def frustum_pass(case):
    """Per splat: does its centre pass the vertex stage's frustum rejects under the case's modelView and projection (float64) - the
    shader's 1.2 w test and GL's clip of the quad's depth, -1 <= ndc.z <= 1 (what removes a splat behind an orthographic camera)?"""
    u = case["uniforms"]
    mv = np.asarray(u["model_view"], np.float64).reshape(4, 4).T
    p = np.asarray(u["projection"], np.float64).reshape(4, 4).T
    c = np.concatenate([case["centers"].astype(np.float64), np.ones((case["centers"].shape[0], 1))], axis=1)
    q = c @ (p @ mv).T
    clip = 1.2 * q[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ndcz = q[:, 2] / q[:, 3]
    return ~((q[:, 2] < -clip) | (q[:, 0] < -clip) | (q[:, 0] > clip) | (q[:, 1] < -clip) | (q[:, 1] > clip)) & (ndcz >= -1.0) & (ndcz <= 1.0)


def boxes_outside(case, positions, margin=1e-3):
    """Per storage block: do all eight corners of the box of its centres satisfy ONE reject of the 1.2 w test by `margin` (ten times
    the relative tolerance block_corner keeps for its fp32 evaluation)?  Then the block test has to declare the block dead."""
    centers = case["centers"].astype(np.float64)
    blocks = (centers.shape[0] + 255) // 256
    out = np.zeros(blocks, bool)
    for b in range(blocks):
        c = centers[np.asarray(positions) // 256 == b]
        lo, hi = c.min(axis=0), c.max(axis=0)
        corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
        q = clip_coordinates(case, corners)
        clip = 1.2 * q[:, 3]
        tol = margin * (np.abs(q[:, :3]).sum(axis=1) + np.abs(clip) + 1.0)
        rej = [q[:, 0] - clip > tol, -q[:, 0] - clip > tol, q[:, 1] - clip > tol, -q[:, 1] - clip > tol, -q[:, 2] - clip > tol, -q[:, 3] > tol]
        out[b] = any(r.all() for r in rej)
    return out


def per_block(flags, positions):
    """Number of set flags per 256-splat storage block; positions = the storage position of every splat."""
    blocks = (len(flags) + 255) // 256
    return np.bincount(np.asarray(positions)[np.asarray(flags, bool)] // 256, minlength=blocks)


# -- the forward error bound of the window depth --------------------------------------------------------------------------------
def window_depth_bound(case):
    """(z, dz) per splat in float64: the window depth 0.5 ndc.z + 0.5 of the centre from the fp32 uniforms, and the forward error
    bound of its fp32 evaluation q = P (MV c), ndc.z = q2 / q3, z = 0.5 ndc.z + 0.5:
      |dq_r| <= g9 (|P| |MV| |c|)_r with g_k = k 2^-24 / (1 - k 2^-24);  d ndc.z <= (dq2 + |ndc.z| dq3) / |q3| (1 + 4 2^-24);
      dz = 0.5 d ndc.z + 2^-24.
    Under per-scene transforms MV is viewMatrix * transform of the splat's scene."""
    u = case["uniforms"]
    f32 = lambda m: np.asarray(m, np.float64).astype(np.float32).astype(np.float64).reshape(4, 4).T
    p = f32(u["projection"])
    n = case["centers"].shape[0]
    c = np.concatenate([case["centers"].astype(np.float64), np.ones((n, 1))], axis=1)
    if case["build"] == "dynamic2":
        view = f32(u["view_matrix"])
        mvs = np.stack([view @ f32(t) for t in u["transforms"]])[case["scene_idx"]]
    else:
        mvs = np.broadcast_to(f32(u["model_view"]), (n, 4, 4))
    v = np.einsum("nrk,nk->nr", mvs, c)
    q = v @ p.T
    mag = np.einsum("nrk,nk->nr", np.abs(mvs), np.abs(c)) @ np.abs(p).T
    eps = 2.0 ** -24
    g9 = 9 * eps / (1 - 9 * eps)
    dq = g9 * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ndcz = q[:, 2] / q[:, 3]
        dndc = (dq[:, 2] + np.abs(ndcz) * dq[:, 3]) / np.abs(q[:, 3]) * (1 + 4 * eps)
    return 0.5 * ndcz + 0.5, 0.5 * dndc + eps
