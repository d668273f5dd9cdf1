"""Scenes of the quadrant-test tests (tests/test_quadrant_ref.py on the CPU, tests/test_gpu_quadrant_test.py on the device): the
smallest frames on which exact_quadrants (csrc/tile_blend.hip) can go wrong - long diagonal ellipses far from their centre, cut
contours that graze a quadrant's corner or the middle of its edge, axis-aligned forms, centres inside and on a quadrant's boundary.

Most frames are 136 x 104 px = 8.5 x 6.5 tiles: the right and the top edge cut a tile, a quadrant and a bin.  Splats are built in
screen space the way surface_cases.layer builds them, generalised to an anisotropic covariance and a roll angle: flat in the
camera's image plane (no extent along the view axis), so that the vertex stage's cov2D is (focal / depth)^2 x the world covariance
+ the 0.3 px^2 kernel, whatever the centre's offset from the axis.  Sizes are given as the half-axes of the cut contour
(`half` = sqrt(8) standard deviations, what max_screen_space_splat_size caps at 1024 px); the kernel puts a floor of
sqrt(8 x 0.3) = 1.55 px under them.

No case holds a record with an inf or a NaN: the vertex stage never marks one visible.  An fp16 covariance that overflows makes
cov2D infinite, l1 - a = inf - inf = NaN, the eigenvector NaN, and `e1x == e1x` fails (project.hip, as in the reference's
shader); a NaN centre fails the rect's `fx0 <= fx1`.  The visible records are K * e / (k h) with |e| = 1 and 1.55 k <= k h <= 1024 k
(k = splat_scale / focal adjustment): finite for any k that does not underflow.  So there is no nan_record case; that
exact_quadrants keeps on a NaN is asserted on a synthetic record in tests/test_quadrant_ref.py.
"""
from dataclasses import dataclass

import numpy as np

import helpers
import surface_cases
from gaussiansplats3d_amd import camera, scenes

W, H = 136, 104
LONG_W, LONG_H = 1056, 72
KERNEL = 0.3                                     # kernel_2d_size: added to both diagonal entries of cov2D
FAMILIES = ["needle_diag", "corner_graze", "axis_aligned", "inside", "random_small"]
NAMES = {"needle_diag": ["needle_diag", "needle_diag_far"], "corner_graze": ["corner_graze"],
         "axis_aligned": ["axis_aligned", "axis_aligned_129x97", "axis_aligned_127x95"],
         "inside": ["inside", "inside_129x97", "inside_127x95"], "random_small": ["random_small_5", "random_small_6"]}


@dataclass
class Case:
    name: str
    w: int
    h: int
    cam: object
    scene: object
    draws: list                  # index arrays: the splats of each draw (the one-splat draws of the hand-made cases; one draw of all)
    order: object = None         # the draw order of the all-splats draw (None: by index)


def splat(cam, at_px, half_long, half_short, angle_deg, depth=4.0):
    """One splat flat in the image plane of `cam` (small_camera: the view axes are the world's), its centre at the window position
    `at_px` (pixel i's centre is at i + 0.5), the cut contour's half-axes (half_long, half_short) px with the long one `angle_deg`
    from +x towards +y.  Returns (centre [3], cov [6])."""
    focal = cam.focal()[1]
    c = cam.position + np.array([(at_px[0] - cam.width / 2.0) * depth / focal, (at_px[1] - cam.height / 2.0) * depth / focal, -depth])
    var = [max(hh * hh / 8.0 - KERNEL, 0.0) * (depth / focal) ** 2 for hh in (half_long, half_short)]
    quarter = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}
    co, si = quarter.get(angle_deg % 360, (np.cos(np.deg2rad(angle_deg)), np.sin(np.deg2rad(angle_deg))))
    vxx, vxy, vyy = co * co * var[0] + si * si * var[1], co * si * (var[0] - var[1]), si * si * var[0] + co * co * var[1]
    return c.astype(np.float32), np.array([vxx, vxy, 0.0, vyy, 0.0, 0.0], dtype=np.float32)


def case_of(name, w, h, parts):
    cam = surface_cases.small_camera(w, h)
    built = [splat(cam, *p) for p in parts]
    centers = np.stack([b[0] for b in built]).astype(np.float32)
    cov = np.stack([b[1] for b in built]).astype(np.float32)
    rgba = np.full((len(built), 4), 255, dtype=np.uint8)                      # opaque and white
    scene = scenes.SplatScene(centers, cov, rgba, np.zeros((len(built), 0), np.float16), 0)
    return Case(name, w, h, cam, scene, [np.array([i], dtype=np.uint32) for i in range(len(built))])


_axes_cache = {}


def record_axes(w, h, half_long, half_short, angle_deg):
    """The two rows (a, b) of the pixel -> ellipse-space map the vertex stage gives this shape, in fp64 from the oracle's record.
    They do not depend on where the splat is (it is flat in the image plane), but they are not the analytic ones: for a needle the
    shader's small eigenvalue l2 = tr / 2 - sqrt(disc) is a difference of two fp32 numbers near 1e5, good to a few per cent."""
    key = (w, h, half_long, half_short, angle_deg)
    if key not in _axes_cache:
        c = case_of("axes", w, h, [((w / 2.0 + 0.3, h / 2.0 + 0.3), half_long, half_short, angle_deg)])
        recs, vis = surface_cases.oracle_records(c.scene, c.cam, w, h)
        assert vis[0]
        _axes_cache[key] = tuple(np.asarray(v[0], np.float64) for v in surface_cases.ref.rec_fields(recs)[2:6])
    return _axes_cache[key]


def graze(w, h, target_px, along, below_cut, side, half_long, half_short, angle_deg):
    """A needle placed so that ONE pixel of a far quadrant passes the fragment rule, by `below_cut`: the pixel centre `target_px`
    lies `along` px from the splat's centre along the long axis and just inside the cut contour on the side `side` (+-1) of it.
    (The centre goes through the vertex stage in fp32: it lands within ~3e-5 px of where it is asked for, i.e. the power at the
    pixel within ~2e-4 of the one asked for.)"""
    ax, ay, bx, by = record_axes(w, h, half_long, half_short, angle_deg)
    flip = np.sign(ax * np.cos(np.deg2rad(angle_deg)) + ay * np.sin(np.deg2rad(angle_deg)))
    u0 = np.hypot(ax, ay) * along * flip
    left = bx * -np.sin(np.deg2rad(angle_deg)) + by * np.cos(np.deg2rad(angle_deg))       # side +1: left of the direction angle_deg
    w0 = side * np.sign(left) * np.sqrt(surface_cases.ref.CUT - below_cut - u0 * u0)
    d = np.linalg.solve(np.array([[ax, ay], [bx, by]]), np.array([u0, w0]))
    return ((target_px[0] - d[0], target_px[1] - d[1]), half_long, half_short, angle_deg)


def needle_diag():
    """One needle per draw.  35 on the 136 x 104 frame: seven angles x half lengths from 200 px to the 1024-px cap (1500 asked for),
    the short half-axis from the kernel's floor to 11 px (4 px standard deviation), centres in and just outside the frame.  18 on
    the 1056 x 72 frame: the centre near one end (inside the vertex stage's 1.2 x centre clip), shallow angles, so that the needle is
    still inside the frame 900 - 1040 px from its centre.  And on both frames needles of the thinnest kind placed so that a single
    corner pixel of a quadrant far along them is inside the cut by 3e-4 .. 4e-3 (graze): where the expanded form of the edge
    minimum - terms of 1e4 that cancel to 5.77 - is wrong by more than that."""
    shorts = [0.0, 2.0, 4.0, 11.3]
    small, k = [], 0
    for ang in (5, 30, 45, 60, 85, 95, 135):
        for half in (200.0, 350.0, 600.0, 1023.0, 1500.0):
            at = [(20.3, 11.8), (70.6, 50.2), (131.4, 97.7), (-9.2, 60.4), (66.1, 110.9), (144.8, -6.3)][k % 6]
            small.append((at, half, shorts[k % 4], ang))
            k += 1
    below = (3e-4, 6e-4, 1e-3, 2e-3, 4e-3)
    # the last pixel of the first row of tile (7, 5), 120 px up a 42-degree needle; the first pixel of the last row of tile (7, 4),
    # 118 px up a 45-degree one; the first pixel of the first row of tile (1, 5), 118 px up a 138-degree one.  (Which way the expanded
    # form errs is a property of the shape - of how m00, m01, m11 happen to round: at 42 and 3.5 degrees it errs upwards.)
    small += [graze(W, H, (127.5, 80.5), 120.0, e, +1, 1023.0, 0.0, 42) for e in below]
    small += [graze(W, H, (112.5, 79.5), 118.0, e, -1, 1500.0, 0.0, 45) for e in below]
    small += [graze(W, H, (16.5, 80.5), 118.0, e, -1, 1023.0, 0.0, 138) for e in below]
    far = []
    for j, (ang, at) in enumerate([(1, (18.4, 20.3)), (2, (25.7, 10.6)), (3.5, (12.2, 6.9)), (5, (-40.3, -6.8)), (0.4, (-80.6, 31.7)),
                                   (-1.5, (30.9, 60.2)), (-3, (9.3, 68.8)), (-4, (-60.5, 78.1)), (2.5, (-99.9, -4.4)),
                                   (179, (1040.2, 18.7)), (178, (1029.6, 12.3)), (176.5, (1046.3, 5.1)), (175, (1100.4, -6.2)),
                                   (181.5, (1020.8, 58.6)), (183, (1050.1, 66.4)), (184, (1120.3, 78.9)), (179.6, (1150.2, 40.3)),
                                   (177.5, (1155.5, -3.9))]):
        far.append((at, [1023.0, 1500.0, 900.0][j % 3], shorts[j % 4], ang))
    # the last pixel of the first row of tile (61, 4) - the frame's partial top row - 940 px up a 3.5-degree needle; the first pixel
    # of the first row of tile (3, 4), 990 px up a 176.5-degree one
    far += [graze(LONG_W, LONG_H, (991.5, 64.5), 940.0, e, +1, 1023.0, 0.0, 3.5) for e in below]
    far += [graze(LONG_W, LONG_H, (48.5, 64.5), 990.0, e, -1, 1023.0, 0.0, 176.5) for e in below]
    return [case_of("needle_diag", W, H, small), case_of("needle_diag_far", LONG_W, LONG_H, far)]


def corner_graze():
    """80 splats, one per draw: the cut contour (distance `half` from the centre along the long axis, which points at the target)
    swept in 0.25-px steps across a corner pixel of a quadrant - all four orientations, two of them in the partial bins of the
    frame's right and top edge - and across the middle of each edge of an interior quadrant.  No step lands on the pixel itself
    (-0.625 .. +0.375): a pixel exactly on the contour would be one nobody can judge."""
    steps = [-0.625, -0.375, -0.125, 0.125, 0.375]
    parts = []
    # (corner pixel's centre, direction from the splat's centre to it): tile (4, 3) lower left, tile (8, 2) upper left [right edge],
    # tile (3, 6) lower right [top edge], tile (2, 1) upper right
    corners = [((64.5, 48.5), 45.0), ((128.5, 47.5), -45.0), ((63.5, 96.5), 135.0), ((47.5, 31.5), 225.0)]
    for (p, ang) in corners:
        for half, short in ((6.0, 6.0), (17.0, 17.0 / 3.0), (40.0, 40.0)):
            for d in steps:
                r = half + d
                at = (p[0] - r * np.cos(np.deg2rad(ang)), p[1] - r * np.sin(np.deg2rad(ang)))
                parts.append((at, half, short, ang))
    # the middle of the four edges of tile (4, 3) (x 64 .. 79, y 48 .. 63), approached head-on by 3 : 1 splats (a round splat's
    # reach along the axes is not its `half`: the shader floors the discriminant of the eigenvalues at 0.1, so l = a +- 0.316)
    edges = [((71.5, 48.5), 90.0, 9.0, 3.0), ((71.5, 63.5), 270.0, 12.0, 4.0), ((64.5, 55.5), 0.5, 30.0, 10.0), ((79.5, 56.5), 180.0 + 0.5, 21.0, 7.0)]
    for (p, ang, half, short) in edges:
        for d in steps:
            r = half + d
            at = (p[0] - r * np.cos(np.deg2rad(ang)), p[1] - r * np.sin(np.deg2rad(ang)))
            parts.append((at, half, short, ang))
    return [case_of("corner_graze", W, H, parts)]


def axis_aligned():
    """Needles along the axes.  The long axis along y gives m01 = 0 exactly (e1 = (0, 1)); the long axis along x does not exist as
    a record with m01 = 0: for b = 0 the shader's eigenvector normalize(vec2(b, l1 - a)) is (0, +-1) or NaN, so such a splat is
    drawn turned or not at all - whatever the vertex stage makes of it is in the case - and 0.01 degrees off the axis it is an
    ordinary needle.  The two odd frames put the screen centre on a pixel centre, exactly, in fp32: 129 x 97 -> (64.5, 48.5), the
    first pixel column and row of a quadrant; 127 x 95 -> (63.5, 47.5), the last ones - there X0 or X1 is exactly 0 (xb == 0)."""
    parts = []
    for at, half, short in (((70.3, -5.2), 300.0, 0.0), ((37.9, 50.1), 1500.0, 3.0), ((128.2, 110.6), 640.0, 0.0), ((64.2, 20.7), 25.0, 2.0)):
        parts.append((at, half, short, 90))
    for at, half, short, ang in (((-7.7, 70.3), 300.0, 0.0, 0.01), ((141.3, 30.1), 1500.0, 3.0, 179.99), ((60.4, 100.9), 640.0, 2.0, 0.01),
                                 ((30.2, 47.9), 200.0, 0.0, 0), ((99.1, 77.4), 200.0, 4.0, 180)):
        parts.append((at, half, short, ang))
    out = [case_of("axis_aligned", W, H, parts)]
    for w, h in ((129, 97), (127, 95)):
        mid = (w / 2.0, h / 2.0)
        out.append(case_of(f"axis_aligned_{w}x{h}", w, h, [(mid, 300.3, 0.0, 90), (mid, 40.3, 5.0, 90), (mid, 300.3, 0.0, 0.01), (mid, 9.3, 9.3, 0),
                                                             ((mid[0], mid[1] - 30.0), 12.3, 3.0, 90), ((mid[0] - 30.0, mid[1]), 12.3, 3.0, 0.01)]))
    return out


def inside():
    """The centre inside a quadrant (qmin = 0), on (within 1e-5 px of) its boundary pixel centre, half a pixel outside it - on a tile
    edge - and on the corner four tiles share; on the two odd frames the centre is exactly on a quadrant's first / last pixel
    centre.  Small splats, 2.5 to 5 px (a round splat much smaller than that is not drawn at all: the floored discriminant makes
    its smaller eigenvalue negative)."""
    parts = []
    for half, short in ((2.5, 2.5), (3.0, 1.0), (5.0, 5.0)):
        for at in ((72.3, 56.7), (64.5, 56.5), (64.0, 56.5), (64.0, 48.0), (79.5, 63.5), (135.6, 103.7)):
            parts.append((at, half, short, 30.0))
    out = [case_of("inside", W, H, parts)]
    for w, h in ((129, 97), (127, 95)):
        out.append(case_of(f"inside_{w}x{h}", w, h, [((w / 2.0, h / 2.0), 2.5, 2.5, 0), ((w / 2.0, h / 2.0), 4.0, 2.0, 60.0)]))
    return out


def random_small():
    """helpers.small_scene(3000, 1, seed) at 150 x 90, seeds 5 and 6: the scenes the surface tests already trust, here for how many
    quadrants the test keeps."""
    import oracle
    from gaussiansplats3d_amd import util
    out = []
    for seed in (5, 6):
        cam = camera.demo_camera("garden", 150, 90)
        scene = helpers.small_scene(3000, 1, seed)
        order = oracle.sort_indexes(np.arange(scene.count, dtype=np.uint32), util.integer_centers(scene.centers), cam.sort_mvp())
        out.append(Case(f"random_small_{seed}", 150, 90, cam, scene, [np.arange(scene.count, dtype=np.uint32)], order))
    return out


_family_cache = {}


def family(name):
    """The cases (frames) of a family: built once, shared, unchanged."""
    if name not in _family_cache:
        _family_cache[name] = {"needle_diag": needle_diag, "corner_graze": corner_graze, "axis_aligned": axis_aligned, "inside": inside,
                               "random_small": random_small}[name]()
        assert [c.name for c in _family_cache[name]] == NAMES[name]
    return _family_cache[name]


def case(name):
    fam = next(f for f in FAMILIES if name in NAMES[f])
    return family(fam)[NAMES[fam].index(name)]


_oracle_cache = {}


def oracle_planes(case):
    """(records, rects, visible) of a case as the CPU oracle's vertex stage forms them (surface_cases.oracle_records), the rects
    restated from project.hip's bound: computed once per case and shared, unchanged."""
    if case.name not in _oracle_cache:
        recs, vis = surface_cases.oracle_records(case.scene, case.cam, case.w, case.h)
        _oracle_cache[case.name] = (recs, oracle_rects(recs, vis, case.w, case.h), vis)
    return _oracle_cache[case.name]


def oracle_rects(recs, vis, w, h):
    """The vertex stage's tile rect (csrc/project.hip) from a record: the basis vectors are b = K a / |a|^2, the extent
    sqrt(b1x^2 + b2x^2) * 1.00001 + 1e-3, the rect the pixel centres inside it, clipped to the frame.  A record whose rect is empty
    is not visible (returned flags are and-ed into `vis` in place)."""
    f = np.float32
    K = f(surface_cases.K_POWER)
    cx, cy, ax, ay, ex, ey, _ = surface_cases.ref.rec_fields(recs)
    with np.errstate(all="ignore"):
        n1, n2 = ax * ax + ay * ay, ex * ex + ey * ey
        b1x, b1y, b2x, b2y = K * ax / n1, K * ay / n1, K * ex / n2, K * ey / n2
        ext_x = np.sqrt(b1x * b1x + b2x * b2x) * f(1.00001) + f(1e-3)
        ext_y = np.sqrt(b1y * b1y + b2y * b2y) * f(1.00001) + f(1e-3)
        fx0, fx1 = np.maximum(np.ceil(cx - ext_x - f(0.5)), 0), np.minimum(np.floor(cx + ext_x - f(0.5)), w - 1)
        fy0, fy1 = np.maximum(np.ceil(cy - ext_y - f(0.5)), 0), np.minimum(np.floor(cy + ext_y - f(0.5)), h - 1)
        ok = vis & (fx0 <= fx1) & (fy0 <= fy1)
    vis &= ok
    t = lambda v: np.where(ok, v, 0).astype(np.int64) // 16
    rects = np.zeros((recs.shape[0], 2), dtype=np.uint32)
    rects[:, 0] = (t(fx0) | (t(fy0) << 16)).astype(np.uint32)
    rects[:, 1] = (t(fx1) | (t(fy1) << 16)).astype(np.uint32)
    return rects
