"""CPU: the host model of SplatRenderMode.TwoD (tests/surfel_ref.py) and its cases (tests/surfel_cases.py).

 * the homography the vertex stage builds is the 2DGS one: a point of the surfel's plane, projected to pixels, is sent back to
   its own plane coordinates by the fragment rule's cross product - checked from first principles in fp64;
 * the cases hold what they promise (both quad branches, splats behind the camera / beyond the far plane / edge-on rejects,
   the ambiguous-pixel cap);
 * every mutation of the chain changes some case's records or frame, so a kernel that carried it could not pass
   tests/test_gpu_surfel.py;
 * the flag and the debug selector are present in the header and in the binding.
"""
import os
import re

import numpy as np
import pytest

import surfel_cases
import surfel_ref
from gaussiansplats3d_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_and_selector_in_header_and_binding():
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define GS_MESH_SURFEL 8u", header)
    assert L.GS_MESH_SURFEL == 8 and not (L.GS_MESH_SURFEL & (L.GS_MESH_COV_HALF | L.GS_MESH_SH_U8 | L.GS_MESH_KEEP_ORDER))
    assert re.search(r"\n \* 15 = \(GS_MESH_SURFEL meshes only", header) and L.GS_DEBUG_RECORDS_2D == 15
    assert re.search(r"#define GS_ABI_VERSION 5\b", header)


def test_homography_maps_a_plane_point_back_to_its_plane_coordinates():
    """T from first principles: the world point p + a L0 + b L1 projects to pixel-index coordinates x = ndc.x W / 2 + (W - 1) / 2
    (the ndc2pix of SplatMaterial2D.js:121-123); with k = x Tw - Tu, l = y Tw - Tv, cross(k, l) is proportional to (a, b, 1)."""
    case = surfel_cases.vertex_case("sh0")
    v = surfel_ref.vertex(case)
    W, H = case["width"], case["height"]
    M = (case["proj"].astype(np.float64).reshape(4, 4).T @ case["view"].astype(np.float64).reshape(4, 4).T)
    rng = np.random.default_rng(1)
    checked = 0
    for i in np.flatnonzero(v["visible"])[:200]:
        if 16 <= i < 28:                                       # edge-on: the map back is singular there
            continue
        sx, sy, _, qx, qy, qz = case["tuples"][i].astype(np.float64)
        qw = np.sqrt(max(0.0, 1 - qx * qx - qy * qy - qz * qz))
        R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                      [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                      [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
        a, b = rng.uniform(-1.5, 1.5, 2)
        world = case["centers"][i].astype(np.float64) + a * sx * R[:, 0] + b * sy * R[:, 1]
        clip = M @ np.array([*world, 1.0])
        if clip[3] < 0.05:
            continue
        x = clip[0] / clip[3] * W / 2 + (W - 1) / 2
        y = clip[1] / clip[3] * H / 2 + (H - 1) / 2
        tu, tv, tw = (v[k][i].astype(np.float64) for k in ("tu", "tv", "tw"))
        p = np.cross(x * tw - tu, y * tw - tv)
        assert abs(p[0] / p[2] - a) < 2e-3 * (1 + abs(a)) and abs(p[1] / p[2] - b) < 2e-3 * (1 + abs(b)), (i, a, b, p)
        # ... and the fragment's depth is the clip w of that point
        assert abs((a * tw[0] + b * tw[1] + tw[2]) - clip[3]) < 1e-3 * abs(clip[3])
        checked += 1
    assert checked > 100


@pytest.mark.parametrize("name", surfel_cases.VERTEX_CASES)
def test_vertex_cases_hold_what_they_promise(name):
    case = surfel_cases.vertex_case(name)
    v = surfel_ref.vertex(case)
    vis = v["visible"]
    drawn = int(vis.sum())
    assert drawn > 400
    square = int((v["branch"][vis] == 1).sum())
    print(f"{name}: drawn {drawn}, AABB branch {square}, parallelogram {drawn - square}")
    assert square >= 0.05 * drawn and drawn - square >= 0.05 * drawn          # both quad branches
    assert not vis[0:16].any()                                                # beyond the far plane, behind the camera
    assert (v["branch"][16:28] == 1).all()                                    # the edge-on ones: thinner than a pixel
    if name == "effects":
        assert not vis[case["scene_idx"] != 0].any()                          # scene 1 invisible, scene 2 below 0.01 opacity
    r = surfel_ref.records(v)
    assert np.isfinite(r[vis, :17].view(np.float32)).all()


def _frame(kind, name, mut=()):
    case, order, dest = (surfel_cases.frame_case if kind == "frame" else surfel_cases.designed_case)(name)
    return surfel_ref.render(case, order, mut, **dest)


@pytest.mark.parametrize("kind,name", [("frame", n) for n in surfel_cases.FRAME_CASES] + [("designed", n) for n in surfel_cases.DESIGNED_CASES])
def test_ambiguous_pixel_cap(kind, name):
    out = _frame(kind, name)
    covered, amb = int(out["covered"].sum()), int((out["ambiguous"] & out["covered"]).sum())
    print(f"{kind} {name}: covered {covered}, ambiguous {amb}")
    assert covered > 0
    assert amb <= surfel_cases.AMBIGUOUS_CAP * covered
    assert (out["frame"][out["covered"] & ~out["ambiguous"]][:, 3] > 0).any()


def test_designed_cases_reach_what_they_are_designed_for():
    v = surfel_ref.vertex(surfel_cases.designed_case("basis_one_pixel")[0])
    assert v["branch"].tolist() == [1, 0, 1, 0] and (v["len"][0] < 1).any() and (v["len"][1] >= 1).all()
    out = _frame("designed", "near_plane_crossing")
    v = out["vertex"]
    x0, y0, x1, y1 = v["pixel_rect"][0]
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    kept, _ = surfel_ref.fragments(v, 0, xs, ys)
    free, _ = surfel_ref.fragments(v, 0, xs, ys, mut=("near_removed",))
    assert (kept > 0).any() and ((free > 0) & (kept == 0)).any()              # depth < 0.2 discards part of the quad
    out = _frame("designed", "termination")
    assert (out["exact"][..., 3] > 1 - 1e-4).sum() > 200                       # saturated pixels in front of the 300
    out = _frame("designed", "destination_between")
    case, order, dest = surfel_cases.designed_case("destination_between")
    plain = surfel_ref.render(case, order)
    assert not np.array_equal(out["frame"][:, 32:], plain["frame"][:, 32:])   # the far surfel is hidden on the right half
    v = surfel_ref.vertex(surfel_cases.designed_case("distance_reject")[0])      # |distance| < 1e-5: gl_Position unwritten
    assert v["visible"].tolist() == [True, False] and v["branch"][1] == 1 and abs(v["distance"][1]) < 1e-5
    for n in (1, 255, 256, 257, 513):
        v = surfel_ref.vertex(surfel_cases.designed_case(f"list_{n}")[0])
        assert v["visible"].all() and (v["rect"] <= 1).all() and v["visible"].size == n     # every entry reaches bin (0, 0)


@pytest.mark.parametrize("mut", surfel_ref.MUTATIONS)
def test_every_mutation_changes_a_case(mut):
    """A kernel carrying the mutation would leave the tolerance of test_gpu_surfel.py on some case: records move by more than
    5e-4 relative / 3e-3 px, or non-ambiguous pixels by more than one 8-bit step."""
    vertex_side = mut in ("factor3_sqrt8", "ifa_omitted", "minpix_never", "minpix_always", "missing_w_negated", "t_transposed",
                          "ndc2pix_minus1_omitted")
    caught = []
    if vertex_side:
        for name in ("sh0", "focal_adjustment"):
            case = surfel_cases.vertex_case(name)
            a, b = surfel_ref.vertex(case), surfel_ref.vertex(case, (mut,))
            both = a["visible"] & b["visible"]
            if (a["visible"] != b["visible"]).any():
                caught.append(name)
                continue
            for key, tol in (("tu", 5e-4), ("tv", 5e-4), ("tw", 5e-4), ("inv", 5e-4)):
                scale = np.linalg.norm(a[key][both], axis=1, keepdims=True)
                if (np.abs(a[key][both] - b[key][both]) > tol * scale).any():
                    caught.append(name)
                    break
    for kind, name in (("frame", "mixed_branches"), ("frame", "opaque"), ("designed", "near_plane_crossing"), ("designed", "rho_balance")):
        ref, got = _frame(kind, name), _frame(kind, name, (mut,))
        clean = ~(ref["ambiguous"] | got["ambiguous"])
        if (np.abs(ref["frame"].astype(int) - got["frame"].astype(int))[clean] > 1).any():
            caught.append(name)
    print(mut, "caught by", caught)
    assert caught


def test_rop8_composite_stays_near_the_fp32_one():
    out = _frame("frame", "translucent")
    rop = surfel_ref.composite_rop8(out["vertex"], out["fragments"], 160, 96)
    diff = np.abs(rop.astype(int) - out["frame"].astype(int))
    print("rop8 vs fp32: equal share", float((diff == 0).mean()), "worst", int(diff.max()))
    assert diff.max() <= 8 and (diff <= 1).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------------
# against the reference's own shader strings run on a real GL (tests/golden/surfel_gl_ref*.npz, tests/tools/make_surfel_golden.py)
# ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = [np.load(os.path.join(ROOT, "tests", "golden", f)) for f in ("surfel_gl_ref.npz", "surfel_gl_ref2.npz")]
MANIFEST = __import__("json").loads(bytes(GOLDEN[0]["manifest"]).decode())
# the figures the 3D vertex-stage check holds a restatement to: 3e-3 px, 5e-4 of a row's norm, one unorm16 unit
FLOOR = {"centre_px": 3e-3, "basis_px": 3e-3, "quad_center_px": 3e-3, "t_rows_rel": 5e-4, "colour_unorm16": 1.0, "ndcz": 5e-4}


def gl_capture(name):
    g = GOLDEN[surfel_cases.VERTEX_CASES.index(name) // 4]
    return g["written_" + name], g["vs_" + name]


def gl_frame(name):
    return GOLDEN[1]["frame_" + name]


@pytest.mark.parametrize("name", surfel_cases.VERTEX_CASES)
def test_model_vertex_stage_against_gl_transform_feedback(name):
    case = surfel_cases.vertex_case(name)
    v = surfel_ref.vertex(case)
    written, cap = gl_capture(name)
    vis = v["visible"]
    assert written[vis].all()                                  # whatever the model draws, the shader wrote gl_Position for
    sel = {k: (a[written] if isinstance(a, np.ndarray) else a) for k, a in v.items()}
    d = surfel_ref.gl_distances(sel, cap, case["width"], case["height"])
    for key, bound in FLOOR.items():
        worst = float(d[key][vis[written]].max())
        print(f"{name} {key}: model to GL {worst:.3e} (recorded {MANIFEST['vertex_distance'][name][key]:.3e})")
        assert worst <= bound and worst <= MANIFEST["vertex_distance"]["worst"][key] * (1 + 1e-6) + 1e-12
    # what the shader wrote and the model does not draw: clipped whole by GL (the quad's depth is the centre's), or a quad whose
    # pixel box holds no pixel centre of the viewport
    extra = written & ~vis
    capx = cap[(~vis)[written]].astype(np.float64)
    cx, cy = (capx[:, 0:8:2] * 0.5 + 0.5) * case["width"], (capx[:, 1:8:2] * 0.5 + 0.5) * case["height"]
    clipped = np.abs(capx[:, 8]) > 1.0
    x0, x1 = np.ceil(cx.min(axis=1) + 2e-3 - 0.5), np.floor(cx.max(axis=1) - 2e-3 - 0.5)
    y0, y1 = np.ceil(cy.min(axis=1) + 2e-3 - 0.5), np.floor(cy.max(axis=1) - 2e-3 - 0.5)
    empty = (np.maximum(x0, 0) > np.minimum(x1, case["width"] - 1)) | (np.maximum(y0, 0) > np.minimum(y1, case["height"] - 1))
    assert int(extra.sum()) == capx.shape[0] and (clipped | empty | ~np.isfinite(cx).all(axis=1)).all()


ALL_FRAMES = [("frame", n) for n in surfel_cases.FRAME_CASES] + [("designed", n) for n in surfel_cases.DESIGNED_CASES if n != "distance_reject"]


@pytest.mark.parametrize("kind,name", ALL_FRAMES)
def test_model_frames_against_gl(kind, name):
    """The model's fp32 composite against GL's RGBA8 frame.  llvmpipe rounds the fragment's colour and alpha to 8 bits BEFORE it
    blends (oracle/raster_oracle.c notes the same for the 3D material), so single surfels sit within one step and deep lists a
    few steps away; the recorded distance is the reference the engine's gate is built on, and the coverage - which pixels any
    fragment reaches - is exact."""
    out = _frame(kind, name)
    gl = gl_frame(name)
    clean = out["covered"] & ~out["ambiguous"]
    d = np.abs(out["frame"].astype(int) - gl.astype(int))
    rec = MANIFEST["frames"][name]
    assert int(d[clean].max()) == rec["fp32_worst"] and rec["uncovered_equal"]
    assert np.array_equal(gl[~out["covered"]], out["frame"][~out["covered"]])
    # (a handful of surfels over a cleared target: only the 8-bit rounding of one source colour and alpha lies between the two)
    alone = out["vertex"]["visible"].sum() <= 4 and name != "destination_between"
    assert rec["fp32_worst"] <= (1 if alone else 8)
    assert ((gl[..., 3] > 0) == (out["frame"][..., 3] > 0))[~out["ambiguous"]].all()


@pytest.mark.parametrize("mut", surfel_ref.MUTATIONS)
def test_every_mutation_is_caught_against_the_gl_golden(mut):
    """Against GL, not against the model itself: a vertex-side mutation leaves the transform feedback by more than the engine's
    tolerance; a fragment-side one moves some non-ambiguous pixel further from GL's frame than the unmutated model is, by more
    than the one step the engine's gate allows."""
    caught = []
    for name in ("sh0", "focal_adjustment"):
        case = surfel_cases.vertex_case(name)
        v = surfel_ref.vertex(case, (mut,))
        ref = surfel_ref.vertex(case)
        written, cap = gl_capture(name)
        sel = {k: (a[written] if isinstance(a, np.ndarray) else a) for k, a in v.items()}
        d = surfel_ref.gl_distances(sel, cap, case["width"], case["height"])
        on = ref["visible"][written]
        if any(float(np.nan_to_num(d[key][on], nan=np.inf).max()) > 4 * FLOOR[key] for key in FLOOR):
            caught.append(name)
    for kind, name in (("frame", "mixed_branches"), ("designed", "near_plane_crossing"), ("designed", "rho_balance"), ("designed", "basis_one_pixel"),
                       ("designed", "one_quadrant")):
        ref, got, gl = _frame(kind, name), _frame(kind, name, (mut,)), gl_frame(name).astype(int)
        clean = ~(ref["ambiguous"] | got["ambiguous"])
        excess = np.abs(got["frame"].astype(int) - gl) - np.abs(ref["frame"].astype(int) - gl)
        if (excess[clean] > 1).any():
            caught.append(name)
    print(mut, "caught against GL by", caught)
    assert caught
