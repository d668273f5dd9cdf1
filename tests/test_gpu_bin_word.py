"""-m gpu: the binner's 4-byte look-up word (csrc/bin_word.hpp) against the 8-byte one it replaces on frames of <= 256 x 256 tiles.

Hand-placed meshes of 512 - 1000 splats in upload order (keep_order: storage block b holds the splats 256 b .. 256 b + 255) are
drawn twice: in a context that chooses the word itself, and in one created under GSPLAT_NO_COMPACT_BIN_WORD=1.  The two draws must
agree bit for bit - frame, visible_splats / tiles16 / tile_entries, every list range and every entry - because the word is an
encoding of one intermediate and nothing that is computed.  Every scene is checked on the CPU first, with the oracle's vertex stage:
the rects follow from oracle.project's basis vectors the way k_project forms them, and the spans, the blocks and the escapes a scene
is named for must really be there.
"""
import numpy as np
import pytest

import helpers
import oracle
from gaussiansplats3d_amd import Context, SplatMesh, camera, scenes, util

pytestmark = pytest.mark.gpu
TILE = 16
MAX_SPAN = 14                          # the widest span the 4-byte word holds (BIN_WORD_MAX_SPAN)
NONE = 0xFFFFFFFF


# -- scenes ---------------------------------------------------------------------------------------------------------------------
def axes(cam):
    mw = np.asarray(cam.matrix_world, dtype=np.float64).reshape(16)
    return mw[0:3], mw[4:7], -mw[8:11]                     # right, up, forward


def aligned(cam, px, py, ext_x, ext_y, depth):
    """One splat whose screen ellipse is axis-aligned: centre at window pixel (px, py) (y up, as the vertex stage counts), reaching
    about ext_x / ext_y px to either side (sqrt(8) standard deviations of the projected Gaussian after the 0.3 px^2 kernel)."""
    right, up, fwd = axes(cam)
    fx, fy = cam.focal()
    centre = cam.position + fwd * depth + right * ((px - 0.5 * cam.width) * depth / fx) + up * ((py - 0.5 * cam.height) * depth / fy)
    sx = np.sqrt(max(ext_x * ext_x / 8.0 - 0.3, 1e-3)) * depth / fx
    sy = np.sqrt(max(ext_y * ext_y / 8.0 - 0.3, 1e-3)) * depth / fy
    sz = 1e-3 * min(sx, sy)
    S = sx * sx * np.outer(right, right) + sy * sy * np.outer(up, up) + sz * sz * np.outer(fwd, fwd)
    return centre.astype(np.float32), np.array([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]], np.float32)


def dots(cam, count, rng, depth=(3.0, 6.0), margin=24.0):
    """`count` splats of ~5 px that are certainly on screen."""
    out = [aligned(cam, rng.uniform(margin, cam.width - margin), rng.uniform(margin, cam.height - margin), 5.0, 5.0, rng.uniform(*depth))
           for _ in range(count)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def behind(cam, count, rng):
    """Splats strictly behind the eye: they draw nothing."""
    _, _, fwd = axes(cam)
    centers = cam.position - fwd * rng.uniform(0.5, 9.0, size=(count, 1)) + rng.normal(size=(count, 3)) * 0.2
    return centers.astype(np.float32), np.tile(np.array([[1e-4, 0, 0, 1e-4, 0, 1e-4]], np.float32), (count, 1))


def scene_of(centers, cov, seed):
    n = centers.shape[0]
    rgba = np.random.default_rng(seed).integers(1, 256, size=(n, 4), dtype=np.uint8)
    rgba[:, 3] = np.maximum(rgba[:, 3], 40)
    return scenes.SplatScene(centers.astype(np.float32), cov.astype(np.float32), rgba, np.zeros((n, 0), np.float16), 0)


W, H = 640, 400                        # 40 x 25 tiles
# the marked splats of the span scene: name -> (index, window px, py, ext_x, ext_y, (span x, span y) it is placed for).  A rect of span
# s starts 8 px into a tile and ends 8 px into the tile s further: ext = 8 s + 0.5, so every edge is half a tile from a tile border
MARKS = {
    "x14": (257, 8 + 8 * 14 + 64, 200.0, 8 * 14 + 0.5, 5.0, (14, 0)),        # the last direct word in x ...
    "x15": (259, 8 + 8 * 15 + 64, 120.0, 8 * 15 + 0.5, 5.0, (15, 0)),        # ... and the first escape
    "y14": (261, 504.0, 8 + 8 * 14 + 48, 5.0, 8 * 14 + 0.5, (0, 14)),
    "y15": (263, 568.0, 8 + 8 * 15 + 48, 5.0, 8 * 15 + 0.5, (0, 15)),
    "frame": (265, 320.0, 200.0, 900.0, 900.0, (39, 24)),                   # covers the whole frame
}


def span_scene():
    """1000 splats, four storage blocks: 0 = 256 dots, all visible (the last one takes slot 255); 1 = even positions visible - the marked
    splats among them - and odd ones behind the eye; 2 = all behind the eye (a dead block); 3 = 232 dots (a partial block)."""
    cam = camera.demo_camera("garden", W, H)
    rng = np.random.default_rng(5)
    c0, v0 = dots(cam, 256, rng)
    c1, v1 = dots(cam, 256, rng)
    cb, vb = behind(cam, 256, rng)
    c1[1::2], v1[1::2] = cb[1::2], vb[1::2]
    for idx, px, py, ex, ey, _ in MARKS.values():
        c1[idx - 256], v1[idx - 256] = aligned(cam, px, py, ex, ey, 2.0 if ex < 800 else 1.0)
    c2, v2 = behind(cam, 256, rng)
    c3, v3 = dots(cam, 232, rng)
    return cam, scene_of(np.concatenate([c0, c1, c2, c3]), np.concatenate([v0, v1, v2, v3]), 5)


def wide_scene(width, height=256):
    """512 splats on a frame `width` px wide: dots, and as the last splat one in the frame's last tile column."""
    cam = camera.demo_camera("garden", width, height)
    rng = np.random.default_rng(width)
    c, v = dots(cam, 512, rng)
    c[511], v[511] = aligned(cam, width - 8.0, 128.0, 3.0, 3.0, 4.0)
    c[1::8], v[1::8] = behind(cam, 64, rng)
    return cam, scene_of(c, v, width)


def oracle_rects(scene, cam, tile_rows=None):
    """(visible bool [n], x0, y0, x1, y1 in 16-px tiles) from the oracle's vertex stage, formed as k_project forms them: the ellipse's
    pixel bounds from the basis vectors, clamped to the frame and the strip."""
    c, cov, rgba, sh = helpers.oracle_inputs(scene)
    ocam = oracle.make_camera(cam.model_view(), cam.projection, cam.position, cam.width, cam.height, 0, 0)
    o = oracle.project(ocam, c, cov, rgba, sh)
    f = np.float32
    ext_x = np.sqrt(o["b1x"] * o["b1x"] + o["b2x"] * o["b2x"]) * f(1.00001) + f(1e-3)
    ext_y = np.sqrt(o["b1y"] * o["b1y"] + o["b2y"] * o["b2y"]) * f(1.00001) + f(1e-3)
    rows = (cam.height + TILE - 1) // TILE
    r0, r1 = (0, rows) if tile_rows is None else tile_rows
    with np.errstate(invalid="ignore"):
        fx0 = np.maximum(np.ceil(o["cx"] - ext_x - f(0.5)), f(0))
        fx1 = np.minimum(np.floor(o["cx"] + ext_x - f(0.5)), f(cam.width - 1))
        fy0 = np.maximum(np.ceil(o["cy"] - ext_y - f(0.5)), f(r0 * TILE))
        fy1 = np.minimum(np.floor(o["cy"] + ext_y - f(0.5)), f(min(cam.height, r1 * TILE) - 1))
        vis = (o["visible"] == 1) & (fx0 <= fx1) & (fy0 <= fy1)
    t = lambda v: np.where(vis, v, 0).astype(np.int64) // TILE
    return vis, t(fx0), t(fy0), t(fx1), t(fy1)


def escapes(x0, y0, x1, y1):
    return (x1 - x0 > MAX_SPAN) | (y1 - y0 > MAX_SPAN) | (x1 > 255) | (y1 > 255)


# -- the two draws --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    """(a context that chooses the word, a context created under the switch that forces the 8-byte word).  The switch is read with the
    draw's other switches, so it stays set while the second context draws: draw_pair sets it around those draws."""
    mp = pytest.MonkeyPatch()
    a = Context(0)
    mp.setenv("GSPLAT_NO_COMPACT_BIN_WORD", "1")
    b = Context(0)
    mp.delenv("GSPLAT_NO_COMPACT_BIN_WORD")
    yield a, b, mp
    mp.undo()
    a.close()
    b.close()


def draw(ctx, scene, cam, order, R, tile_rows=None):
    mesh = SplatMesh(ctx, scene.count, 0, False, keep_order=True)
    mesh.build(scene.centers, scene.cov, scene.rgba, None)
    mesh.set_camera(cam)
    mesh.update_render_indexes(order, R)
    frame, stats = mesh.render(tile_rows=tile_rows)
    ranges, entries, slots = mesh.bin_lists(tile_rows, list_bin_px=int(stats.list_bin_px))
    _, rects, vis = mesh.debug_records()
    out = dict(frame=frame, stats=(int(stats.visible_splats), int(stats.tiles16), int(stats.tile_entries)), ranges=ranges, entries=entries,
               slots=slots, rects=rects, vis=vis, narrow=mesh.bin_word_narrow(), list_px=int(stats.list_bin_px))
    mesh.dispose()
    return out


def draw_pair(contexts, scene, cam, order, R, tile_rows=None, narrow=True):
    """Both draws, compared; returns the first.  narrow: the word the first context must report (the second always the 8-byte one)."""
    a, b, mp = contexts
    got = draw(a, scene, cam, order, R, tile_rows)
    mp.setenv("GSPLAT_NO_COMPACT_BIN_WORD", "1")
    try:
        ref = draw(b, scene, cam, order, R, tile_rows)
    finally:
        mp.delenv("GSPLAT_NO_COMPACT_BIN_WORD")
    assert got["narrow"] == narrow and ref["narrow"] is False
    assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
    assert got["list_px"] == ref["list_px"]
    assert np.array_equal(got["vis"], ref["vis"]) and np.array_equal(got["slots"], ref["slots"])
    assert np.array_equal(got["rects"][got["vis"]], ref["rects"][ref["vis"]])
    assert np.array_equal(got["ranges"], ref["ranges"])
    assert np.array_equal(got["entries"], ref["entries"])
    assert got["frame"].tobytes() == ref["frame"].tobytes()
    return got


def depth_order(scene, cam):
    return oracle.sort_indexes(np.arange(scene.count, dtype=np.uint32), util.integer_centers(scene.centers), cam.sort_mvp())


def device_fields(rects):
    return rects[:, 0] & 0xFFFF, rects[:, 0] >> 16, rects[:, 1] & 0xFFFF, rects[:, 1] >> 16


def check_span_scene(scene, cam, tile_rows=None):
    """The CPU side: the oracle's rects have the spans, blocks and escapes the scene is built for.  Returns (vis, x0, y0, x1, y1)."""
    vis, x0, y0, x1, y1 = oracle_rects(scene, cam, tile_rows)
    if tile_rows is None:
        for name, (idx, _, _, _, _, (sx, sy)) in MARKS.items():
            assert vis[idx] and (x1[idx] - x0[idx], y1[idx] - y0[idx]) == (sx, sy), (name, x0[idx], y0[idx], x1[idx], y1[idx])
        esc = escapes(x0, y0, x1, y1) & vis
        assert sorted(np.flatnonzero(esc).tolist()) == sorted(MARKS[k][0] for k in ("x15", "y15", "frame"))
        f = MARKS["frame"][0]
        assert (x0[f], y0[f], x1[f], y1[f]) == (0, 0, W // TILE - 1, H // TILE - 1)                # the whole frame
    assert vis[0:256].all()                                                                        # slot 255 is taken
    assert not vis[512:768].any()                                                                  # a dead block
    odd = np.arange(257, 512, 2)
    assert vis[256:512:2].all() and not vis[odd[~np.isin(odd, [m[0] for m in MARKS.values()])]].any()   # invisible positions of a live block
    assert vis[768:].all() and scene.count == 1000
    return vis, x0, y0, x1, y1


def check_device_rects(got, vis, x0, y0, x1, y1):
    """... and the device formed the same ones (so the escapes the oracle names are the escapes the kernels took)."""
    assert np.array_equal(got["vis"], vis)
    d = device_fields(got["rects"])
    for mine, theirs in zip(d, (x0, y0, x1, y1)):
        assert np.array_equal(mine[vis], theirs[vis])


# -- the cases ------------------------------------------------------------------------------------------------------------------
def test_spans_at_the_edge_of_the_word_full_and_dead_blocks_against_the_oracle_frame(contexts):
    cam, scene = span_scene()
    vis, x0, y0, x1, y1 = check_span_scene(scene, cam)
    order = depth_order(scene, cam)
    got = draw_pair(contexts, scene, cam, order, scene.count)
    check_device_rects(got, vis, x0, y0, x1, y1)
    assert got["slots"][255] == 255 and got["slots"][0] == 0                                       # block 0: every slot, in order
    assert (got["slots"][512:768] == NONE).all() and got["slots"][267] == NONE and got["slots"][266] != NONE
    assert got["stats"][0] == int(vis.sum())
    assert got["stats"][1] == int(((x1 - x0 + 1) * (y1 - y0 + 1))[vis].sum())                      # tiles16 over the listed splats
    c, cov, rgba, sh = helpers.oracle_inputs(scene)
    ocam = oracle.make_camera(cam.model_view(), cam.projection, cam.position, cam.width, cam.height, 0, 0)
    fb, _, amb, frags = oracle.render(ocam, c, cov, rgba, sh, order)
    assert frags > 1000
    print(helpers.compare_frames(got["frame"], fb, amb, "span scene"))


def test_a_strip_clips_escaping_rects(contexts):
    """Tile rows 6 .. 18 of 25: the frame-covering splat keeps its 39-tile x span (still an escape, now 12 rows high); the 16-row rect is
    cut to the strip's 12 rows and becomes a direct word; x15 lies outside the strip or inside it with its escape intact."""
    cam, scene = span_scene()
    rows = (6, 18)
    check_span_scene(scene, cam)
    vis, x0, y0, x1, y1 = oracle_rects(scene, cam, rows)
    f, tall = MARKS["frame"][0], MARKS["y15"][0]
    assert vis[f] and (x0[f], y0[f], x1[f], y1[f]) == (0, rows[0], W // TILE - 1, rows[1] - 1)
    assert vis[tall] and y1[tall] - y0[tall] < 15 and (y0[tall] == rows[0] or y1[tall] == rows[1] - 1)   # clipped, no longer an escape
    assert (escapes(x0, y0, x1, y1) & vis).sum() >= 1 and 50 < vis.sum() < scene.count
    got = draw_pair(contexts, scene, cam, depth_order(scene, cam), scene.count, tile_rows=rows)
    check_device_rects(got, vis, x0, y0, x1, y1)
    assert got["frame"].shape[0] == (rows[1] - rows[0]) * TILE


def test_a_short_list_with_a_repeat_and_an_index_past_the_end(contexts):
    """The caller's list names 700 positions: the marked splats, one of them twice, and once the index n (past the end: it draws
    nothing).  visible_splats and tiles16 count LISTED splats: the repeat counts twice."""
    cam, scene = span_scene()
    vis, x0, y0, x1, y1 = check_span_scene(scene, cam)
    n = scene.count
    order = depth_order(scene, cam)
    R = 700
    order = order[:R].copy()
    marks = [m[0] for m in MARKS.values()]
    keep = order[~np.isin(order, marks)]
    order = np.concatenate([keep[:R - len(marks) - 2], np.array(marks + [MARKS["x15"][0], n], dtype=np.uint32)]).astype(np.uint32)
    assert order.shape[0] == R < n and (order == n).sum() == 1 and (order == MARKS["x15"][0]).sum() == 2
    got = draw_pair(contexts, scene, cam, order, R)
    listed = order[order < n]
    assert got["stats"][0] == int(vis[listed].sum())
    assert got["stats"][1] == int(((x1 - x0 + 1) * (y1 - y0 + 1))[listed][vis[listed]].sum())


def test_tile_column_255_of_a_4096_px_frame(contexts):
    cam, scene = wide_scene(4096)
    vis, x0, y0, x1, y1 = oracle_rects(scene, cam)
    assert vis[511] and x1[511] == 255 and x1.max() == 255 and not (escapes(x0, y0, x1, y1) & vis).any()
    assert 300 < vis.sum() < 512 and not vis[0:256].all()                                          # invisible positions in live blocks
    got = draw_pair(contexts, scene, cam, depth_order(scene, cam), scene.count, narrow=True)
    check_device_rects(got, vis, x0, y0, x1, y1)


def test_a_frame_of_257_tile_columns_uses_the_wide_word(contexts):
    cam, scene = wide_scene(4112)
    vis, x0, y0, x1, y1 = oracle_rects(scene, cam)
    assert vis[511] and x1[511] == 256 and (cam.width + TILE - 1) // TILE == 257
    got = draw_pair(contexts, scene, cam, depth_order(scene, cam), scene.count, narrow=False)      # chosen, and reported as chosen
    check_device_rects(got, vis, x0, y0, x1, y1)
