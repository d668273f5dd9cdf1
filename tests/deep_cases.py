"""Designed scenes of the chunked-composite tests (tests/test_deep_ref.py on the CPU, tests/test_gpu_deep_edges.py on the device):
frames that put NAMED survivor counts into NAMED quadrants, with loud markers on both sides of every chunk edge a case targets.

Built on quadrant_cases.splat - one splat flat in the image plane of surface_cases.small_camera at a window position.  Every splat
(but the 20-px stack of `saturating`, which reaches three neighbouring bins) lies wholly inside one 32-px bin, and a bin's splats are given one depth each along the view axis, 0.001 apart (distinct integer
centres: a sort would have no ties), in the order the bin's list is to have; the draw order handed to the engine is that order.

  fill     round, cut contour 4.5 px, centred in its quadrant + one of 32 jitters (screened so that no pixel centre lies near the
           fill's cut contour: offsets()), 8-bit alpha 1 or 2.  It stays more than a pixel inside its quadrant: its rect is that one tile and no
           neighbour is reached (a splat whose cut contour covered a whole quadrant would bulge into the neighbours: the two
           wishes exclude each other, and the survivor counts need the second).  Pixels under its middle saturate after a few
           thousand of them; pixels near its rim see alphas down to 0.018 / 255, and the quadrant's corners stay at T = 1 - so
           the quadrant never saturates and the chunks' stop rule never fires unless a case asks for it.
  pair     the same, 13 x 4.5 px upright, centred on the seam of quadrants q and q + 2: one entry, a survivor of both.
  marker   round, 3 px, in a corner of the quadrant ((3.5, 3.5) px from it) where no fill reaches, alpha 200 (blue: 100).  For a
           chunk edge b the survivors b - 2, b - 1, b of the quadrant are blue, RED, GREEN on the same spot: a drop, a repeat or a
           swap at the edge moves the red or the green channel by tens of 1/255 at the marker's pixels (the repeat at the pixels
           1 - 2 px from its centre, where alpha is ~0.3: at the centre the three leave T = 0.03).  The checked pixels are all
           pixels of the bin's live quadrants; the marker pixels (a marker spot's own pixel and its four neighbours) must hold no
           ambiguous fragment.
"""
from dataclasses import dataclass, field

import numpy as np

import bin_lists_ref
import deep_ref
import quadrant_cases
import surface_cases
import surface_ref as ref
from gaussiansplats3d_amd import scenes

W, H = 256, 160                                   # 8 x 5 = 40 blend bins
EDGE_W, EDGE_H = 272, 176                         # 16 mod 32 both ways: 9 x 6 bins, the last column and the top row are half bins
D0, STEP, HIDE = 2.0, 0.001, 60.0
FILL_HALF, MARK_HALF, PAIR_HALF, WIDE_HALF, JITTER = 4.5, 3.0, 13.0, 20.0, 0.5
CORNERS = [(3.5, 3.5), (12.5, 3.5), (3.5, 12.5), (12.5, 12.5)]
RED, GREEN, BLUE = (255, 0, 0), (0, 255, 0), (0, 0, 255)
MARK_ALPHA, BLUE_ALPHA = 200, 100
NAMES = ["ladder_a", "ladder_b", "ladder_c", "tail", "cap", "sparse", "edge", "saturating", "depth"]


@dataclass
class Target:
    """What a case says about one quadrant of one bin."""
    S: int                       # survivors
    edges: list                  # the chunk edges (survivor b - 1 | b) its markers sit on
    saturating: bool = False


@dataclass
class Case:
    name: str
    w: int
    h: int
    cam: object
    scene: object
    order: np.ndarray            # the draw order: back to front
    targets: dict                # {(bx, by): {q: Target}}
    list_len: dict               # {(bx, by): entries of the bin's list}
    hidden: np.ndarray = None    # bool [n]: the splat lies behind the destination's plane (depth)
    items: list = None           # per splat: (window position, half long, half short, angle, rgba, hidden)
    depth_index: np.ndarray = None   # per splat: its place in its bin's list
    strips: list = field(default_factory=list)
    dest_depth: np.ndarray = None
    list_shift: int = 1          # 32-px list bins: a blend bin's list is its own


_offsets = {}


def offsets(w, h, half_long, half_short, angle, count=32, margin=0.02, reach=1, spread=JITTER):
    """`count` jitters (dx, dy) in [-spread, spread]^2, from a seeded generator, at which a splat of this shape - centred on a
    pixel corner + the jitter - has no pixel centre within `margin` (in power) of its cut contour: no fragment of it is ambiguous
    (the shape's axes are the oracle's, quadrant_cases.record_axes: for small round splats the shader's floored discriminant moves
    the contour by tenths of a pixel).  reach: how many 32-px bins around its own the lattice of pixel centres covers."""
    key = (w, h, half_long, half_short, angle, count, margin, reach, spread)
    if key not in _offsets:
        ax, ay, bx, by = quadrant_cases.record_axes(w, h, half_long, half_short, angle)
        g = np.arange(-32 * reach, 32 * reach) + 0.5
        gy, gx = (v.ravel() for v in np.meshgrid(g, g, indexing="ij"))
        rng, out = np.random.default_rng(7), []
        while len(out) < count:
            j = rng.uniform(-spread, spread, size=2)
            u, v = ax * (gx - j[0]) + ay * (gy - j[1]), bx * (gx - j[0]) + by * (gy - j[1])
            if np.abs(u * u + v * v - ref.CUT).min() > margin:
                out.append(j)
        _offsets[key] = np.array(out)
    return _offsets[key]


class Bin:
    """The list of one bin, near -> far."""

    def __init__(self, bx, by, rng, w=W, h=H):
        self.bx, self.by, self.rng, self.w, self.h = bx, by, rng, w, h
        self.items, self.counts = [], [0, 0, 0, 0]

    def _origin(self, q):
        return self.bx * 32 + (q & 1) * 16, self.by * 32 + (q >> 1) * 16

    def fill(self, q, n=1, hidden_every=0):
        x0, y0 = self._origin(q)
        table = offsets(self.w, self.h, FILL_HALF, FILL_HALF, 0)
        js = table[self.rng.integers(0, table.shape[0], size=n)]
        cols, als = self.rng.integers(40, 256, size=(n, 3)), self.rng.integers(1, 3, size=n)
        for k in range(n):
            hidden = bool(hidden_every) and self.counts[q] % hidden_every == hidden_every - 1
            self.items.append(((x0 + 8.0 + js[k, 0], y0 + 8.0 + js[k, 1]), FILL_HALF, FILL_HALF, 0,
                               (int(cols[k, 0]), int(cols[k, 1]), int(cols[k, 2]), int(als[k])), hidden))
            self.counts[q] += 1

    def pair(self, q, n=1):
        """n entries that survive in q and in q + 2."""
        x0, y0 = self._origin(q)
        table = offsets(self.w, self.h, PAIR_HALF, FILL_HALF, 90)
        js = table[self.rng.integers(0, table.shape[0], size=n)]
        cols = self.rng.integers(40, 256, size=(n, 3))
        for k in range(n):
            self.items.append(((x0 + 8.0 + js[k, 0], y0 + 16.0 + js[k, 1]), PAIR_HALF, FILL_HALF, 90,
                               (int(cols[k, 0]), int(cols[k, 1]), int(cols[k, 2]), 1), False))
            self.counts[q] += 1
            self.counts[q + 2] += 1

    def marker(self, q, corner, colour, alpha=MARK_ALPHA, hidden=False):
        x0, y0 = self._origin(q)
        cx, cy = CORNERS[corner]
        self.items.append(((x0 + cx, y0 + cy), MARK_HALF, MARK_HALF, 0, tuple(colour) + (alpha,), hidden))
        self.counts[q] += 1

    def fill_to(self, q, k, hidden_every=0):
        assert self.counts[q] <= k, (q, self.counts[q], k)
        self.fill(q, k - self.counts[q], hidden_every)

    def edge(self, q, b, corner, have_b=True, hidden_every=0, hide=None):
        """Fills up to survivor b - 3, then blue, red, green as survivors b - 2, b - 1, b.  hide: "red" / "green" - that marker
        lies behind the destination's depth; then a visible pair (red, green) goes to b - 4, b - 3 on the next corner."""
        if hide and not have_b:
            hide = "red"                                   # (an edge at S has no survivor b: the one that is there is hidden)
        if hide:
            self.fill_to(q, b - 4, hidden_every)
            self.marker(q, (corner + 1) % 4, RED)
            self.marker(q, (corner + 1) % 4, GREEN)
        self.fill_to(q, b - 2, hidden_every)
        self.marker(q, corner, BLUE, BLUE_ALPHA)
        self.marker(q, corner, RED, hidden=hide == "red")
        if have_b:
            self.marker(q, corner, GREEN, hidden=hide == "green")

    def quadrant(self, q, S, edges, hidden_every=0, hide=None, corners=None):
        """S survivors of q with markers on `edges` (an edge at S: no survivor b); corners: where each edge's markers go.  With a
        hidden marker the trio sits on a right-hand corner (1, 3: under the destination's plane, every pixel of it) and the visible
        pair on the left-hand corner after it (2, 0: depth 1)."""
        for i, b in enumerate(edges):
            corner = corners[i] if corners else (2 * i + 1 if hide else i) % 4
            self.edge(q, b, corner, have_b=b < S, hidden_every=hidden_every, hide=hide)
        self.fill_to(q, S, hidden_every)

    def interleave(self):
        """Spread the quadrants' survivors through the list (round robin): the order among entries of different quadrants is
        free, a quadrant's own order is kept.  Only for lists of single-quadrant entries."""
        per = [[it for it in self.items if self._q_of(it) == q] for q in range(4)]
        assert sum(len(p) for p in per) == len(self.items)
        out, at = [], [0, 0, 0, 0]
        while len(out) < len(self.items):
            for q in range(4):
                if at[q] < len(per[q]):
                    out.append(per[q][at[q]])
                    at[q] += 1
        self.items = out

    def _q_of(self, it):
        x, y = it[0][0] - self.bx * 32, it[0][1] - self.by * 32
        return (1 if x >= 16 else 0) + (2 if y >= 16 else 0) if it[1] != PAIR_HALF else -1


def splats(cam, at, half_long, half_short, upright, depth):
    """quadrant_cases.splat for arrays of round or upright (90 degrees) shapes: (centres [n, 3], cov [n, 6]) - the same
    expressions (tests/test_deep_ref.py compares the two)."""
    focal = cam.focal()[1]
    at, depth = np.asarray(at, np.float64), np.asarray(depth, np.float64)
    c = cam.position + np.stack([(at[:, 0] - cam.width / 2.0) * depth / focal, (at[:, 1] - cam.height / 2.0) * depth / focal, -depth], axis=1)
    var = [np.maximum(np.asarray(hh, np.float64) ** 2 / 8.0 - quadrant_cases.KERNEL, 0.0) * (depth / focal) ** 2 for hh in (half_long, half_short)]
    vxx, vyy = np.where(upright, var[1], var[0]), np.where(upright, var[0], var[1])
    z = np.zeros_like(vxx)
    return c.astype(np.float32), np.stack([vxx, z, z, vyy, z, z], axis=1).astype(np.float32)


def assemble(name, w, h, bins, targets, **kw):
    cam = surface_cases.small_camera(w, h)
    items = [it for b in bins for it in b.items]
    depth = np.concatenate([D0 + STEP * np.arange(len(b.items)) for b in bins])
    hidden = np.array([it[5] for it in items], dtype=bool)
    assert all(it[3] in (0, 90) for it in items)
    centers, cov = splats(cam, np.array([it[0] for it in items]), np.array([it[1] for it in items]), np.array([it[2] for it in items]),
                          np.array([it[3] == 90 for it in items]), depth + np.where(hidden, HIDE, 0.0))
    rgba = np.array([it[4] for it in items], dtype=np.uint8)
    scene = scenes.SplatScene(centers, cov, rgba, np.zeros((len(items), 0), np.float16), 0)
    order = np.argsort(-depth, kind="stable").astype(np.uint32)                       # back to front by the list's own depth
    return Case(name, w, h, cam, scene, order, targets, {(b.bx, b.by): len(b.items) for b in bins}, hidden=hidden, items=items,
                depth_index=np.concatenate([np.arange(len(b.items)) for b in bins]), **kw)


def _ladder(counts, seed, bin_at=(3, 2), **kw):
    """One bin; counts: {q: (S, edges)}."""
    b = Bin(*bin_at, np.random.default_rng(seed))
    for q, (S, edges) in counts.items():
        b.quadrant(q, S, edges, **kw)
    b.interleave()
    return b, {bin_at: {q: Target(S, edges) for q, (S, edges) in counts.items()}}


def ladder_a():
    b, t = _ladder({0: (1023, [1023]), 1: (1024, [1024]), 2: (1025, [1024]), 3: (1281, [1024, 1280])}, 101)
    return assemble("ladder_a", W, H, [b], t)


LADDER_B = {0: (2048, [1024, 2048]), 1: (2049, [1280, 2048]), 2: (4096, [2560, 4096]), 3: (4097, [1536, 4096])}


def ladder_b():
    b, t = _ladder(LADDER_B, 102)
    return assemble("ladder_b", W, H, [b], t)


def ladder_c():
    """5120 / 5121, one survivor, and a live quadrant with none: no chunk, its pixels the clear value."""
    b, t = _ladder({0: (5120, [4096, 5120]), 1: (5121, [3072, 5120]), 2: (1, [])}, 103)
    t[(3, 2)][3] = Target(0, [])
    return assemble("ladder_c", W, H, [b], t)


def tail():
    """26 624 (31 bounded chunks, nothing for chunk 31), 26 625 (one survivor in chunk 31) and 30 000 in a list of 56 630 <=
    GS_DEEP_LIST_CAP: 26 622 upright pairs are survivors of quadrants 0 and 2 both.  In the 30 000 the edge 27 648 is marked too:
    where chunk 31 would end if it were bounded like the others."""
    b = Bin(4, 1, np.random.default_rng(104))
    b.pair(0, 1022)
    for q, k in ((0, 1), (2, 3)):                          # (an early edge, marked in both; corners the pairs do not reach)
        b.marker(q, k, BLUE, BLUE_ALPHA); b.marker(q, k, RED); b.marker(q, k, GREEN)
    b.pair(0, 26622 - 1025 - 0)
    assert b.counts[0] == b.counts[2] == 26622
    b.marker(0, 0, BLUE, BLUE_ALPHA); b.marker(0, 0, RED)
    b.marker(2, 2, BLUE, BLUE_ALPHA); b.marker(2, 2, RED); b.marker(2, 2, GREEN)
    b.quadrant(1, 30000, [5120, 26624, 27648])
    t = {(4, 1): {0: Target(26624, [1024, 26624]), 2: Target(26625, [1024, 26624]), 1: Target(30000, [5120, 26624, 27648]), 3: Target(0, [])}}
    return assemble("tail", W, H, [b], t)


def cap():
    """A list of exactly GS_DEEP_LIST_CAP = 65 536 entries and, in another bin, 65 537: two marked quadrants each, the other two
    make the length."""
    bins, t = [], {}
    for at, n, seed in (((1, 1), 65536, 105), ((6, 3), 65537, 106)):
        b = Bin(*at, np.random.default_rng(seed))
        b.quadrant(0, 4097, [1024, 4096])
        b.quadrant(1, 5121, [2048, 5120])
        rest = n - 4097 - 5121
        b.quadrant(2, rest // 2, [26624])
        b.quadrant(3, rest - rest // 2, [])
        b.interleave()
        assert len(b.items) == n
        bins.append(b)
        t[at] = {0: Target(4097, [1024, 4096]), 1: Target(5121, [2048, 5120]), 2: Target(rest // 2, [26624]), 3: Target(rest - rest // 2, [])}
    return assemble("cap", W, H, bins, t)


SPARSE_AT_1024 = 40 * 1024 + 512 + 32             # list position of survivor 1024: the middle of a window in the middle of range 40


def sparse_positions():
    """List positions of quadrant 0's 1500 survivors in the 60 000-entry list: five runs of 100 consecutive entries (more than 64
    survivors inside two 64-entry windows: the queue carries), a run of 100 around survivor 1024, the rest singles."""
    runs = [np.arange(s, s + 100) for s in (3010, 11030, 19050, 27070, 35090)]
    mid = np.arange(SPARSE_AT_1024 - 20, SPARSE_AT_1024 + 80)
    taken = np.concatenate(runs)
    free = np.setdiff1d(np.arange(0, SPARSE_AT_1024 - 20), taken)
    singles = free[np.linspace(0, free.shape[0] - 1, 1024 - 20 - taken.shape[0]).astype(np.int64)]
    behind = np.arange(SPARSE_AT_1024 + 80, 60000)
    later = behind[np.linspace(0, behind.shape[0] - 1, 1500 - 1024 - 80).astype(np.int64)]
    pos = np.sort(np.concatenate([taken, singles, mid, later]))
    assert pos.shape[0] == 1500 and np.unique(pos).shape[0] == 1500 and pos[1024] == SPARSE_AT_1024
    return pos


def sparse():
    at = (2, 3)
    own = Bin(*at, np.random.default_rng(107))
    own.quadrant(0, 1500, [1024, 1280])
    other = Bin(*at, np.random.default_rng(108))
    n_other = 60000 - 1500
    for q, S in ((1, n_other // 3), (2, n_other // 3), (3, n_other - 2 * (n_other // 3))):
        other.quadrant(q, S, [])
    other.interleave()
    pos = sparse_positions()
    items = [None] * 60000
    for p, it in zip(pos, own.items):
        items[p] = it
    rest = iter(other.items)
    own.items = [it if it is not None else next(rest) for it in items]
    t = {at: {0: Target(1500, [1024, 1280]), 1: Target(n_other // 3, []), 2: Target(n_other // 3, []), 3: Target(n_other - 2 * (n_other // 3), [])}}
    return assemble("sparse", W, H, [own], t)


def edge():
    """272 x 176: bin (8, 5) - last column, top row - has one live quadrant, bin (8, 2) - last column - two, and the strips
    (0, 5) | (5, 11) cut bin (8, 2) between them.  Upright pairs reach from the live quadrant 0 into quadrant 2."""
    top = Bin(8, 5, np.random.default_rng(109), EDGE_W, EDGE_H)
    top.pair(0, 300)                                       # (their upper half is outside the frame)
    top.quadrant(0, 4097, [1024, 4096])
    mid = Bin(8, 2, np.random.default_rng(110), EDGE_W, EDGE_H)
    mid.pair(0, 900)
    mid.quadrant(0, 4097, [1024, 4096])
    mid.quadrant(2, 4097, [1280, 4096], corners=[2, 3])
    t = {(8, 5): {0: Target(4097, [1024, 4096])}, (8, 2): {0: Target(4097, [1024, 4096]), 2: Target(4097, [1280, 4096])}}
    return assemble("edge", EDGE_W, EDGE_H, [top, mid], t, strips=[(0, 5), (5, 11)])


def saturating():
    """Quadrant 0: 1330 survivors, then - inside chunk 2 = [1280, 1536) - 48 opaque splats of 20 px that take every pixel of
    the quadrant below 1e-4, then 3000 more.  (The wide ones reach the neighbouring quadrants and bins as well: 48 survivors there.)"""
    at = (3, 2)
    b = Bin(*at, np.random.default_rng(111))
    b.edge(0, 1024, 0)
    b.edge(0, 1280, 1)
    b.fill_to(0, 1330)
    x0, y0 = b._origin(0)
    j = offsets(W, H, WIDE_HALF, WIDE_HALF, 0, count=1, margin=0.004, reach=2)[0]
    for _ in range(48):
        b.items.append(((x0 + 8.0 + j[0], y0 + 8.0 + j[1]), WIDE_HALF, WIDE_HALF, 0, (255, 255, 255, 255), False))
        b.counts = [n + 1 for n in b.counts]
    b.edge(0, 2048, 2)                                      # (loud, and behind the stack: nothing of it may show)
    b.fill_to(0, 1378 + 3000)
    b.quadrant(3, 4097 + 48, [1024, 4096], corners=[3, 2])  # (corners the stack does not reach)
    t = {at: {0: Target(4378, [1024, 1280], saturating=True), 1: Target(48, []), 2: Target(48, []), 3: Target(4097 + 48, [1024, 4096])}}
    return assemble("saturating", W, H, [b], t)


def depth():
    """ladder_b under a destination depth: the right half of every quadrant holds a plane that hides every third fill and one marker
    of each red / green pair (hidden splats lie 60 behind their place in the order), the left half holds depth 1 (nothing hidden).
    The edge's blue / red / green trio sits on a right-hand corner, every pixel of it under the plane: the hidden marker shows
    nowhere, its partner does.  Hidden survivors still count towards the chunk edges.  Each edge also carries a visible red / green
    pair as survivors b - 4, b - 3, on a left-hand corner."""
    b = Bin(3, 2, np.random.default_rng(112))
    for q, (S, edges) in LADDER_B.items():
        b.quadrant(q, S, edges, hidden_every=3, hide="red" if q & 1 else "green")
    b.interleave()
    c = assemble("depth", W, H, [b], {(3, 2): {q: Target(S, e) for q, (S, e) in LADDER_B.items()}})
    z = ref.window_depth(c.scene.centers, *view_proj(c.cam))
    vis_z, hid_z = z[~c.hidden], z[c.hidden]
    assert vis_z.size and hid_z.size and vis_z.max() < hid_z.min()
    plane = np.float32(0.5 * (vis_z.max() + hid_z.min()))
    d = np.ones((c.h, c.w), dtype=np.float32)
    d[:, (np.arange(c.w) % 16) >= 8] = plane
    c.dest_depth = d
    return c


_cache = {}


def case(name):
    """Built once, shared, unchanged."""
    if name not in _cache:
        _cache[name] = globals()[name]()
    return _cache[name]


# -- glue ---------------------------------------------------------------------------------------------------------------------------
def view_proj(cam):
    return (np.asarray(cam.model_view(), np.float64).astype(np.float32).reshape(16).tolist(),
            np.asarray(cam.projection, np.float64).astype(np.float32).reshape(16).tolist())


_planes = {}


def oracle_planes(c):
    """(records with colours, rects, visible) of a case from the CPU oracle's vertex stage (surface_cases.oracle_records, the
    restatement the other cases files use) - no device."""
    if c.name not in _planes:
        recs, vis = surface_cases.oracle_records(c.scene, c.cam, c.w, c.h)
        u16 = lambda v: np.floor(v.astype(np.float32) / np.float32(255.0) * np.float32(65535.0) + np.float32(0.5)).astype(np.uint32)
        r, g, b_ = (u16(c.scene.rgba[:, k]) for k in range(3))
        recs[:, 6] = r | (g << 16)
        recs[:, 7] = b_ | (recs[:, 7] & np.uint32(0xFFFF0000))
        rects = quadrant_cases.oracle_rects(recs, vis, c.w, c.h)
        _planes[c.name] = (recs, rects, vis)
    return _planes[c.name]


def cpu_draw(c, with_dest=True, unorm24=False):
    """surface_ref.Draw of the case's full frame without a device: the oracle's records, the binner's host model for the lists."""
    recs, rects, vis = oracle_planes(c)
    list_px = 16 << c.list_shift
    lists_x, list_rows = (c.w + list_px - 1) // list_px, (c.h + list_px - 1) // list_px
    slots = np.where(vis, np.arange(vis.shape[0]), ref.NONE).astype(np.uint32)
    lists = bin_lists_ref.expected_lists(c.order, c.scene.count, vis, rects, slots, c.list_shift, lists_x, 0, list_rows)
    z = ref.window_depth(c.scene.centers, *view_proj(c.cam))
    return ref.Draw(width=c.w, height=c.h, list_shift=c.list_shift, lists_x=lists_x, list_row_begin=0, ranges=lists.ranges,
                    entries=lists.entries, slots=slots, recs=recs, rects=rects, vis=vis, z=z,
                    dest_depth=c.dest_depth if with_dest else None, unorm24=unorm24)


def quads_of(draw, rows=None):
    """{(bx, by, q): deep_ref.Quad} of every live quadrant of every bin with a list."""
    smap = draw.splat_of_slot()
    out = {}
    for bx, by in deep_ref.bins_with_lists(draw, rows):
        for q in range(4):
            m = deep_ref.quadrant(draw, bx, by, q, rows, smap)
            if m is not None:
                out[(bx, by, q)] = m
    return out


def marker_pixels(c, quad):
    """bool [p]: the pixels of a targeted quadrant under the middle of a marker spot (the spot's own pixel and its four neighbours)."""
    out = np.zeros(quad.px.shape[0], dtype=bool)
    t = c.targets.get((quad.bx, quad.by), {}).get(quad.q)
    if t is None or not t.edges:
        return out
    x0, y0 = quad.bx * 32 + (quad.q & 1) * 16, quad.by * 32 + (quad.q >> 1) * 16
    for cx, cy in CORNERS:
        out |= np.hypot(quad.px + 0.5 - (x0 + cx), quad.py + 0.5 - (y0 + cy)) < 1.1
    return out


# -- a drawn mesh (the GPU tests and tests/tools/deep_child.py) ------------------------------------------------------------------------
class Rig:
    """One mesh per case, 32-px list bins ($GSPLAT_LIST_SHIFT is read when the mesh is created), the case's own draw order."""

    def __init__(self, ctx, c):
        import os
        from gaussiansplats3d_amd import SplatMesh
        s = c.scene
        had = os.environ.get("GSPLAT_LIST_SHIFT")
        os.environ["GSPLAT_LIST_SHIFT"] = str(c.list_shift)
        try:
            self.mesh = SplatMesh(ctx, s.count, 0)
        finally:
            if had is None:
                del os.environ["GSPLAT_LIST_SHIFT"]
            else:
                os.environ["GSPLAT_LIST_SHIFT"] = had
        self.case = c
        self.mesh.build(s.centers, s.cov, s.rgba, None)
        self.mesh.set_camera(c.cam)
        self.mesh.update_render_indexes(c.order, s.count)
        self.dest, self.unorm24 = None, False

    def set_destination(self, depth=None, unorm24=False):
        self.dest, self.unorm24 = depth, unorm24
        if depth is None:
            self.mesh.set_destination()
        else:
            self.mesh.set_destination(depth=depth, depth_unorm24=unorm24)

    def draw(self, rows=None):
        return self.mesh.render(tile_rows=rows)

    def quads(self, rows=None):
        """The model of the LAST draw, from its own intermediates."""
        d = surface_cases.draw_of(self.mesh, self.case.scene.centers, tile_rows=rows, dest_depth=self.dest, unorm24=self.unorm24)
        assert int(self.mesh.last_stats().list_bin_px) == 16 << self.case.list_shift
        return d, quads_of(d, rows)

    def pairs(self, rows=None):
        """(splat, quadrant) pairs per bin of the last draw: {(bx, by): pairs} (gs_mesh_debug_read what = 4)."""
        st = self.mesh.blend_bin_stats(rows)
        b0 = 0 if rows is None else (rows[0] * 16) // 32
        assert not (st[..., 1] & 1).any()
        return {(bx, by + b0): int(st[by, bx, 1]) // 2 for by in range(st.shape[0]) for bx in range(st.shape[1])}

    def close(self):
        self.mesh.dispose()


def check_frame(frame, Q, w, row0=0, chunks=None, what=""):
    """A frame (or a strip: row 0 = pixel row `row0`) against the model, every pixel: the pixels of the modelled quadrants within
    the per-pixel tolerance, every other pixel the clear value.  Returns (complaints, worst error / tolerance, largest tolerance)."""
    bad, worst, tol = [], 0.0, 0.0
    covered = np.zeros(frame.shape[:2], dtype=bool)
    for key, m in Q.items():
        b, wr, t = deep_ref.compare_quadrant(frame, row0, m, chunks, what)
        bad += b
        worst, tol = max(worst, wr), max(tol, t)
        covered[m.py - row0, m.px] = True
    stray = ~covered & (frame != 0).any(axis=-1)
    if stray.any():
        y, x = (int(v[0]) for v in np.nonzero(stray))
        bad.append(f"{what}: {int(stray.sum())} pixels outside every list are not clear, first ({x}, {y + row0}) = {frame[y, x].tolist()}")
    return bad, worst, tol


def check_pairs(pairs, Q, deep_bins=(), what=""):
    """Per bin: the pairs the draw composited against the model's prediction - sum of S_q where no quadrant saturates, the bounds of
    deep_ref.walk_bounds otherwise (deep_bins: the bins the deep pass composited)."""
    lo, hi = {}, {}
    for (bx, by, q), m in Q.items():
        a, b = deep_ref.walk_bounds(m, (bx, by) in deep_bins)
        lo[(bx, by)], hi[(bx, by)] = lo.get((bx, by), 0) + a, hi.get((bx, by), 0) + b
    bad = [f"{what} bin {k}: {pairs.get(k, 0)} pairs, the model says {lo.get(k, 0)} .. {hi.get(k, 0)}"
           for k in sorted(set(pairs) | set(lo)) if not lo.get(k, 0) <= pairs.get(k, 0) <= hi.get(k, 0)]
    return bad


def expected_members(pairs, c, deep_min=4096, deep_factor=3, rows=None):
    """The bins the schedule makes members of the deep pass from the per-bin pairs of the draw before (blend_schedule_ref: cost =
    2 x pairs over the bins of the frame, or of the strip of tile rows `rows`; every bin of these frames is in the head of the order)."""
    import blend_schedule_ref as sched
    r0, r1 = (0, (c.h + 15) // 16) if rows is None else rows
    b0, b1 = (r0 * 16) // 32, (min(r1 * 16, c.h) + 31) // 32
    cols = (c.w + 31) // 32
    bins = [(bx, by) for by in range(b0, b1) for bx in range(cols)]
    s = sched.schedule([2 * pairs.get(b, 0) for b in bins], cols, len(bins), 0, 0, deep_min, deep_factor)
    if not any(v >= s.trigger for v in s.costs):
        return set()
    return {b for b, v in zip(bins, s.costs) if v >= s.thr}


def closed_share(Q, bins=None):
    """(low, high, quadrants on an edge) chunk partials the per-bin kernel closes in the bins `bins` (default: all) - non-saturating
    quadrants by deep_ref.predicted_closed; a saturating quadrant closes the chunks in front of the one it stops in."""
    quads = [m for (bx, by, q), m in Q.items() if bins is None or (bx, by) in bins]
    calm = [m for m in quads if m.non_saturating()]
    low, high, on_edge = deep_ref.predicted_closed(calm)
    for m in quads:
        if not m.non_saturating():
            a, b = deep_ref.walk_bounds(m, False)
            ca, cb = deep_ref.chunk_of(a - 1), deep_ref.chunk_of(b - 1)
            assert ca == cb, "the case leaves open in which chunk the quadrant stops"
            low, high = low + ca, high + ca
    return low, high, on_edge
