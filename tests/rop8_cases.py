"""Designed scenes of the ROP8 draw modes' tests (tests/test_rop8_ref.py on the CPU, tests/test_gpu_rop8_edges.py on the device): frames
that put NAMED list lengths, survivor counts and stop counts on the edges of k_tile_blend_rop8's index logic (csrc/tile_blend.hip) -
batches of 256 list entries walked from the list's end, the partial batch first, four groups of 64 per batch in descending order,
a stop count per wave inside a batch the workgroup shares - with loud markers on both sides of every targeted edge.

Built on deep_cases.Bin (one bin's list, near -> far, one depth per entry 0.001 apart, the draw order handed to the engine),
quadrant_cases.splat and surface_cases.small_camera; every jitter comes from deep_cases.offsets, so no pixel centre lies near a cut
contour.  A list is written BY POSITION here (Bin8.pad_to / trio_at): a batch edge is a property of the list, not of a quadrant.

  fill     deep_cases' fill (round, cut contour 4.5 px, mid-quadrant) with an 8-bit alpha of 8 .. 40: each one moves an 8-bit target
           by steps (deep_cases' alphas 1 and 2 leave q8 unchanged).  A quadrant's corners stay at T = 1: fills never saturate it.
  faint    alpha 1 .. 3: below 1/64 at every pixel, never counted by the bounded walk's pass 1.
  trio     markers blue, RED, GREEN (3 px, alpha 100 / 200 / 200) of ONE quadrant on one spot at list entries e - 2, e - 1, e for a
           targeted edge e (a multiple of 256: batch edge; of 64: group edge): a drop, a repeat, a swap or a reversed order at the
           edge moves the spot's pixels by tens of steps.
  stack    `count` opaque white round splats, cut contour 64 px, centred on a quadrant: the quadrant's farthest pixel gets alpha
           >= 0.88 from each, so 8 of them take every pixel of it from T = 1 below 1e-7 - and fewer than 6 leave it above 1e-5: a
           stop that falls between two tests of the cadence, one candidate.  The other quadrants of the bin (alpha down to 0.3 at
           their far corners) and the bins around it get 8 survivors they do not saturate under.  `cover` is the same with a cut
           contour of 128 px on the bin's centre: all four quadrants alike.
Every case but `lengths`, `edge8` and `shared` targets the one bin (3, 2) of a 256 x 160 frame; a targeted bin holds <= 1100 entries."""
import numpy as np

import deep_cases
import surface_ref as ref
from deep_cases import BLUE, BLUE_ALPHA, CORNERS, EDGE_H, EDGE_W, GREEN, H, MARK_HALF, RED, W, Target, assemble   # noqa: F401

FILL_HALF, PAIR_HALF = deep_cases.FILL_HALF, deep_cases.PAIR_HALF
STACK_HALF, COVER_HALF = 64.0, 128.0
AT = (3, 2)
LENGTHS = [1, 255, 256, 257, 512, 513, 1025, 320, 321, 384, 385, 449]     # last batches of 1, 255, 256, 1, 256, 1, 1, 64, 65, 128, 129, 193
NAMES = ["lengths", "survivors", "edge8", "stop8", "stop_before", "stop_group2", "stop_batch_last", "still_staged", "stop_last_test",
         "faint_pile", "dest", "shared"]
# the mutations of rop8_ref.mutations() each case is there to catch: {case: {mutation name: the mode it is caught in}}
CATCHES = {
    "lengths": {"drop batch edge - 1": "full", "drop batch edge": "full", "duplicate batch edge": "full", "swap batch edge": "full",
                "drop group edge - 1": "full", "drop group edge": "full", "duplicate group edge": "full", "swap group edge": "full",
                "partial batch nearest": "full", "survivors ascending inside a group": "full", "alpha unrounded": "full"},
    "survivors": {"drop batch edge": "bounded", "swap group edge": "bounded"},
    "stop8": {"every wave takes wave 0's stop": "bounded", "skip the b_stop batch": "bounded", "c_stop -8": "bounded", "c_stop -1": "bounded",
              "c_stop +1": "bounded", "c_stop +8": "bounded"},
    "stop_before": {"c_stop -1": "bounded", "c_stop +1": "bounded", "c_stop -8": "bounded", "c_stop +8": "bounded",
                    "skip the b_stop batch": "bounded"},
    "stop_group2": {"c_stop -1": "bounded", "c_stop +1": "bounded", "cadence restarts at every batch": "bounded"},
    "stop_batch_last": {"c_stop -1": "bounded", "c_stop -8": "bounded"},
    "faint_pile": {"1/64 rule ignored": "bounded"},
    "dest": {"start from 0": "full", "re-admit a depth-rejected fragment": "full"},
}
ONLY_COUNTERS = ("c_stop", "cadence restarts")   # invisible in the bounded mode's colour BY DESIGN (what they drop or add lies behind
                                                 # T <= 1e-6): only the walk counters can show them


class Bin8(deep_cases.Bin):
    """deep_cases.Bin with fills an 8-bit target can see, written by list position."""

    def __init__(self, bx, by, rng, w=W, h=H):
        super().__init__(bx, by, rng, w, h)
        self.turn = 0

    def fill8(self, q, n=1, alphas=(8, 41), hidden_every=0):
        before = len(self.items)
        self.fill(q, n, hidden_every)
        for k in range(before, len(self.items)):
            pos, hl, hs, ang, rgba, hidden = self.items[k]
            self.items[k] = (pos, hl, hs, ang, rgba[:3] + (int(self.rng.integers(*alphas)),), hidden)

    def faint(self, q, n=1):
        self.fill8(q, n, alphas=(1, 4))

    def pair8(self, q, n=1):
        before = len(self.items)
        self.pair(q, n)
        for k in range(before, len(self.items)):
            pos, hl, hs, ang, rgba, hidden = self.items[k]
            self.items[k] = (pos, hl, hs, ang, rgba[:3] + (int(self.rng.integers(8, 41)),), hidden)

    def pad_to(self, pos, qs=(0, 1, 2, 3), **kw):
        """Fills, one quadrant of `qs` after the other, until the list holds `pos` entries."""
        assert len(self.items) <= pos, (len(self.items), pos)
        while len(self.items) < pos:
            self.fill8(qs[self.turn % len(qs)], 1, **kw)
            self.turn += 1

    def trio_at(self, q, e, corner, qs=(0, 1, 2, 3), hide=None, **kw):
        """blue, red, green of quadrant q at the list entries e - 2, e - 1, e.  hide: "red" / "green" lies behind the destination's
        depth plane (a right-hand corner: every pixel of the spot is under the plane)."""
        self.pad_to(e - 2, qs, **kw)
        self.marker(q, corner, BLUE, BLUE_ALPHA)
        self.marker(q, corner, RED, hidden=hide == "red")
        self.marker(q, corner, GREEN, hidden=hide == "green")

    def wide(self, q, count, half, rgba=(255, 255, 255, 255)):
        """`count` round splats of cut contour `half` px centred on quadrant q (None: on the bin): survivors of all four quadrants."""
        x0, y0 = self._origin(0)
        cx, cy = (x0 + 16.0, y0 + 16.0) if q is None else (self._origin(q)[0] + 8.0, self._origin(q)[1] + 8.0)
        j = wide_offset(self.w, self.h, half, cx, cy)
        for _ in range(count):
            self.items.append(((cx + j[0], cy + j[1]), half, half, 0, tuple(rgba), False))
            self.counts = [c + 1 for c in self.counts]

    def stack(self, q, count=8):
        self.wide(q, count, STACK_HALF)


_wide = {}


def wide_offset(w, h, half, cx, cy, margin=4.0 * ref.ETA, tries=400):
    """deep_cases.offsets' screening for a splat too large for it (a contour of hundreds of pixels always passes near SOME centre of
    an unbounded lattice): the jitter, from a seeded generator, that keeps every pixel centre OF THE FRAME furthest from the cut
    contour of a round splat of cut contour `half` px at (cx, cy) - the first one that keeps them `margin` (in power) away."""
    key = (w, h, half, cx, cy)
    if key not in _wide:
        import quadrant_cases
        ax, ay, bx, by = quadrant_cases.record_axes(w, h, half, half, 0)
        gy, gx = (v.ravel() + 0.5 for v in np.meshgrid(np.arange(h), np.arange(w), indexing="ij"))
        rng, best = np.random.default_rng(7), (-1.0, None)
        for _ in range(tries):
            j = rng.uniform(-deep_cases.JITTER, deep_cases.JITTER, size=2)
            u, v = ax * (gx - cx - j[0]) + ay * (gy - cy - j[1]), bx * (gx - cx - j[0]) + by * (gy - cy - j[1])
            gap = float(np.abs(u * u + v * v - ref.CUT).min())
            if gap > best[0]:
                best = (gap, j)
            if gap > margin:
                break
        _wide[key] = best[1]
    return _wide[key]


def _targets(b, edges):
    """{q: Target} of a bin: the builder's own survivor counts and the targeted list positions {q: [e]}."""
    return {q: Target(b.counts[q], sorted(edges.get(q, []))) for q in range(4)}


def _case(name, bins, targets, w=W, h=H, **kw):
    c = assemble(name, w, h, bins, targets, **kw)
    c.dest_rgba = None
    c.stops = {}                                   # {(bx, by, q): (survivors composited, last batch)} the bounded walk is designed to have
    return c


def destination_colour(w, h, seed=5):
    """A colour plane no splat colour resembles: smooth ramps + noise, alpha anywhere."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = np.stack([(x * 3 + y) % 256, (y * 5 + 40) % 256, (x + 2 * y) % 256, (x * 2 + y * 3) % 256], axis=-1)
    return ((d + rng.integers(0, 16, size=d.shape)) % 256).astype(np.uint8)


# -- list lengths ---------------------------------------------------------------------------------------------------------------------
def edges_of_length(n):
    """The edges a list of n entries is marked on: every batch edge with an entry behind it, the group edges 64 and 192 of batch 0
    and the last group edge inside the last batch."""
    out = [e for e in range(256, n, 256)]
    out += [e for e in (64, 192) if e < n]
    first = 256 * ((n - 1) // 256)
    inner = [e for e in range(first + 64, n, 64)]
    if first and inner:
        out.append(inner[-1])
    return sorted(set(out))


def lengths():
    """Twelve bins, one list length each (LENGTHS); every other bin of the frame has n = 0."""
    bins, t = [], {}
    for i, n in enumerate(LENGTHS):
        at = (i % 8, 2 * (i // 8))
        b = Bin8(*at, np.random.default_rng(200 + i))
        edges = {}
        for k, e in enumerate(edges_of_length(n)):
            if e - 2 < len(b.items):
                continue                                   # (no room in front of it: n = 1)
            q = (k + i) % 4
            b.trio_at(q, e, (k // 4 + q) % 4)
            edges.setdefault(q, []).append(e)
        b.pad_to(n)
        assert len(b.items) == n
        bins.append(b)
        t[at] = _targets(b, edges)
    return _case("lengths", bins, t)


# -- survivors per quadrant ------------------------------------------------------------------------------------------------------------
def survivors():
    """n = 800.  Quadrant 3 has no survivor at all; quadrant 0 has none in the whole batch 1 (entries 256 .. 511); 40 upright pairs are
    one entry and a survivor of quadrants 0 and 2 both."""
    b = Bin8(*AT, np.random.default_rng(220))
    b.trio_at(0, 64, 0, qs=(0, 1, 2))
    b.pad_to(250, qs=(0, 1, 2))
    b.trio_at(1, 256, 1, qs=(1, 2))
    b.pad_to(506, qs=(1, 2))
    b.trio_at(2, 512, 2, qs=(1, 2))
    b.pad_to(600, qs=(0, 1, 2))
    b.pair8(0, 40)
    b.trio_at(0, 768, 3, qs=(0, 1, 2))
    b.pad_to(800, qs=(0, 1, 2))
    return _case("survivors", [b], {AT: _targets(b, {0: [64, 768], 1: [256], 2: [512]})})


def edge8():
    """deep_cases' 272 x 176 frame: bin (8, 5) - last column, top row - has one live quadrant, bin (8, 2) two; the strips (0, 5) |
    (5, 11) cut bin (8, 2) between its tile rows, so half its waves are not live in either."""
    top = Bin8(8, 5, np.random.default_rng(221), EDGE_W, EDGE_H)
    top.pair8(0, 30)                                       # (their upper half is outside the frame)
    top.trio_at(0, 256, 0, qs=(0,))
    top.trio_at(0, 512, 3, qs=(0,))
    top.pad_to(600, qs=(0,))
    mid = Bin8(8, 2, np.random.default_rng(222), EDGE_W, EDGE_H)
    mid.pair8(0, 60)
    mid.trio_at(0, 256, 0, qs=(0, 2))
    mid.trio_at(2, 512, 2, qs=(0, 2))
    mid.pad_to(600, qs=(0, 2))
    t = {(8, 5): {0: Target(top.counts[0], [256, 512])}, (8, 2): {0: Target(mid.counts[0], [256]), 2: Target(mid.counts[2], [512])}}
    return _case("edge8", [top, mid], t, w=EDGE_W, h=EDGE_H, strips=[(0, 5), (5, 11)])


# -- bounded stops -----------------------------------------------------------------------------------------------------------------------
def _finish(b, n, loud_behind=True):
    """A trio of quadrant 0 right behind whatever the list holds (loud, and behind the stop: nothing of it may show), fills to n."""
    if loud_behind:
        for colour in (BLUE, RED, GREEN):
            b.marker(0, 0, colour)
    b.pad_to(n)


def stop8():
    """Quadrant 0 stops at survivor 8 - its first test - in batch 0 of three while quadrants 1 .. 3 never saturate (b_stop < last).
    Quadrant 1 ends with S a multiple of 8, quadrant 2 with S not a multiple of 8; quadrant 3 is marked on both batch edges."""
    b = Bin8(*AT, np.random.default_rng(230))
    b.stack(0)
    for colour in (BLUE, RED, GREEN):
        b.marker(0, 0, colour)
    b.trio_at(3, 256, 3)
    b.trio_at(3, 512, 2)
    b.pad_to(700)
    while b.counts[1] % 8:
        b.fill8(1)
    while b.counts[2] % 8 != 5:
        b.fill8(2)
    c = _case("stop8", [b], {AT: _targets(b, {3: [256, 512]})})
    last = (len(b.items) - 1) // 256
    c.stops = {AT + (0,): (8, 0), AT + (1,): (b.counts[1], last), AT + (2,): (b.counts[2], last), AT + (3,): (b.counts[3], last)}
    return c


def _stop_in_batch_1(name, stack_at, seed, n=700, in_batch_0=64):
    """Batch 0: `in_batch_0` survivors of quadrant 0.  Batch 1 belongs to quadrant 0 alone up to and including the stack at the list
    entries stack_at .. stack_at + 7: quadrant 0 stops at survivor in_batch_0 + (stack_at - 256) + 8, the stack's last, with c_stop =
    stack_at - 248."""
    b = Bin8(*AT, np.random.default_rng(seed))
    b.trio_at(1, 64, 1)
    while b.counts[0] < in_batch_0:
        b.pad_to(len(b.items) + 1)
    b.pad_to(256, qs=(1, 2, 3))
    assert b.counts[0] == in_batch_0
    b.trio_at(0, 320, 2, qs=(0,))                            # a group edge of batch 1 in front of the stop: it shows
    b.pad_to(stack_at, qs=(0,))
    b.stack(0)
    _finish(b, n)
    k = in_batch_0 + (stack_at - 256) + 8
    assert k % 8 == 0
    c = _case(name, [b], {AT: _targets(b, {0: [320], 1: [64]})})
    last = (n - 1) // 256
    c.stops = {AT + (0,): (k, 1)}
    c.stops.update({AT + (q,): (b.counts[q], last) for q in (1, 2, 3)})
    return c


def stop_before():
    """c_stop = 128 = before[2]: the stop is the last survivor of group 1 of batch 1, group 2 gives nothing."""
    return _stop_in_batch_1("stop_before", 376, 231)


def stop_group2():
    """c_stop = 164: inside group 2 of batch 1.  Batch 0 holds 60 survivors of quadrant 0 - not a multiple of 8: the stop, at survivor
    224 of the LIST, is no test of a cadence that restarted with the batch (that one would see four of the stack at its 160th
    survivor of the batch and stop at its 168th: survivor 228)."""
    return _stop_in_batch_1("stop_group2", 412, 232, in_batch_0=60)


def stop_batch_last():
    """c_stop = 256: the stop is entry 511, the last entry of batch 1, all of it quadrant 0's."""
    return _stop_in_batch_1("stop_batch_last", 504, 233)


def still_staged():
    """All four quadrants stop at survivor 16 in batch 0 of three: pass 1 ends with batch 0 staged and pass 2 reuses it."""
    b = Bin8(*AT, np.random.default_rng(234))
    b.pad_to(32)
    b.wide(None, 8, COVER_HALF)
    _finish(b, 600)
    c = _case("still_staged", [b], {AT: _targets(b, {})})
    c.stops = {AT + (q,): (16, 0) for q in range(4)}
    return c


def stop_last_test():
    """Quadrant 0 stops at the last test of the last batch: the stack is the list's last 8 entries and its last is survivor S."""
    b = Bin8(*AT, np.random.default_rng(235))
    b.trio_at(0, 512, 1)
    b.pad_to(688)
    while b.counts[0] % 8:
        b.fill8(0)
    b.stack(0)
    c = _case("stop_last_test", [b], {AT: _targets(b, {0: [512]})})
    last = (len(b.items) - 1) // 256
    c.stops = {AT + (q,): (b.counts[q], last) for q in range(4)}
    return c


FAINT_PILE = 1056


def faint_pile():
    """1056 faint covering splats (cut contour 128 px on the bin's centre, alpha 3: 0.0104 .. 0.0118, below 1/64 everywhere) in front
    of four half-opaque covering layers (alpha 153), four more faint ones, and then three loud white layers and a trio per quadrant.
    In exact arithmetic the pile alone leaves T = 1.6e-5 at the bin's corners and the four layers take it to 8e-7: a pass 1 that
    ignored the 1/64 rule would stop at survivor 1064 and the white layers would not show.  The rule counts the four layers only (T =
    0.05): the walk never stops, and they show, by ten steps.  (A pile of 600 would leave an exact T of 2e-3: with layers thin
    enough for something to show behind them no wrong kernel would stop either - the pile is as deep as the mutation needs.)"""
    b = Bin8(*AT, np.random.default_rng(236))
    b.wide(None, FAINT_PILE, COVER_HALF, rgba=(30, 50, 40, 3))
    b.wide(None, 4, COVER_HALF, rgba=(60, 60, 60, 153))
    b.wide(None, 4, COVER_HALF, rgba=(30, 50, 40, 3))
    b.wide(None, 3, COVER_HALF, rgba=(255, 255, 255, 255))
    for q in range(4):
        for colour in (BLUE, RED, GREEN):
            b.marker(q, q, colour)
    b.pad_to(1090)
    c = _case("faint_pile", [b], {AT: _targets(b, {})})
    c.stops = {AT + (q,): (b.counts[q], 4) for q in range(4)}
    return c


# -- the destination -----------------------------------------------------------------------------------------------------------------------
def dest():
    """A thin list (n = 300, batches of 256 and 44) over a destination: a colour plane everywhere - most pixels of the frame are reached
    by no splat - and a depth plane over the right half of every quadrant that hides every third fill and one marker of the trio at
    each targeted edge (256: red, 64: green, 192: red)."""
    b = Bin8(*AT, np.random.default_rng(240))
    b.trio_at(0, 64, 1, hide="green", hidden_every=3)
    b.trio_at(1, 192, 3, hide="red", hidden_every=3)
    b.trio_at(2, 256, 1, hide="red", hidden_every=3)
    b.pad_to(300, hidden_every=3)
    c = _case("dest", [b], {AT: _targets(b, {0: [64], 1: [192], 2: [256]})})
    z = ref.window_depth(c.scene.centers, *deep_cases.view_proj(c.cam))
    vis_z, hid_z = z[~c.hidden], z[c.hidden]
    assert vis_z.size and hid_z.size and vis_z.max() < hid_z.min()
    d = np.ones((c.h, c.w), dtype=np.float32)
    d[:, (np.arange(c.w) % 16) >= 8] = np.float32(0.5 * (vis_z.max() + hid_z.min()))
    c.dest_depth = d
    c.dest_rgba = destination_colour(c.w, c.h)
    return c


# -- 64-px list bins -----------------------------------------------------------------------------------------------------------------------
def shared():
    """GSPLAT_LIST_SHIFT = 2: the four blend bins (2, 2), (3, 2), (2, 3), (3, 3) walk ONE list of 1000 entries, each keeping the
    250 that reach it; a batch of the list holds about 64 entries of each bin."""
    bins, t = [], {}
    for i, at in enumerate(((2, 2), (3, 2), (2, 3), (3, 3))):
        b = Bin8(*at, np.random.default_rng(250 + i))
        b.trio_at(i, 128, i)
        b.pad_to(250)
        bins.append(b)
        t[at] = _targets(b, {})
    c = _case("shared", bins, t, list_shift=2)
    c.list_len = {at: 1000 for at in t}
    return c


_cache = {}


def case(name):
    """Built once, shared, unchanged."""
    if name not in _cache:
        _cache[name] = globals()[name]()
    return _cache[name]


cpu_draw, marker_pixels = deep_cases.cpu_draw, deep_cases.marker_pixels


# -- a drawn mesh (the GPU tests and tests/tools/rop8_child.py) ------------------------------------------------------------------------------
class Rig(deep_cases.Rig):
    def set_destination(self, depth=None, unorm24=False, rgba=None):
        self.dest, self.unorm24, self.rgba = depth, unorm24, rgba
        if depth is None and rgba is None:
            self.mesh.set_destination()
        else:
            self.mesh.set_destination(depth=depth, rgba=rgba, depth_unorm24=unorm24)

    def draw_of(self, rows=None):
        """surface_ref.Draw of the LAST draw, from its own intermediates."""
        import surface_cases
        d = surface_cases.draw_of(self.mesh, self.case.scene.centers, tile_rows=rows, dest_depth=self.dest, unorm24=self.unorm24)
        assert int(self.mesh.last_stats().list_bin_px) == 16 << self.case.list_shift
        return d

    def stats(self, rows=None):
        """{(bx, by): (entries scanned, pairs composited)} of every bin of the last draw (gs_mesh_debug_read what = 4)."""
        st = self.mesh.blend_bin_stats(rows)
        b0 = 0 if rows is None else (rows[0] * 16) // 32
        assert not (st[..., 1] & 1).any()
        return {(bx, by + b0): (int(st[by, bx, 0]), int(st[by, bx, 1]) // 2) for by in range(st.shape[0]) for bx in range(st.shape[1])}
