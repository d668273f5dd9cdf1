"""Host model (numpy, fp64) of the composite once a quadrant is more than one chunk deep (include/gsplat_hip.h, "The composite";
csrc/gs_internal.hpp, CHUNKED COMPOSITE; csrc/tile_blend.hip: bin_body, k_deep_scan, k_deep_plan, deep_unit, k_deep_fold).

Its inputs are a draw's own intermediates, as surface_ref's are: list ranges, entries, records, rects, slot-of-splat
(gs_mesh_debug_read what = 2 / 8 / 0 / 1 / 9) in a surface_ref.Draw, plus the destination depth plane when one is set.

Per (32-px bin, 16 x 16 quadrant) the ordered SURVIVORS are the entries of the bin's list whose quadrant test keeps the quadrant
(quadrant_ref.kernel_test32, the fp32 restatement of quadrant_mask & exact_quadrants; the designed scenes keep every pair out of
quadrant_ref's band, so the test and the truth agree and the model says how many pairs were in the band).  Their number is S_q.
The chunks cut THAT list - fragments the fragment rule or the depth test discards at a pixel still count.

The value of a pixel is the plain front-to-back composite of its kept fragments in fp64: the survivors of its quadrant with
power < CUT whose depth passes.  In exact arithmetic the two-level fold (chunks from T = 1, merged near -> far) IS the plain
composite - "over" is associative - so this is what both executors must produce; the chunks matter for rounding and for the stop
rule only.  The model also gives T after every chunk edge.

Per-pixel tolerance, in 1/255, derived (not fitted):
    0.5                              the final unorm8 rounding
    255 DELTA                        surface_ref's argument: alphas with relative error <= eps move a composite by <= eps, whatever
                                     the depth of the list (sum_j T_{j-1} a_j eps = eps (1 - T))
    255 x 1e-4 x (chunks + 1)        the stop rule: a chunk stops once every pixel of the quadrant holds T <= 1e-4 (what it leaves
                                     out weighs <= 1e-4), and so does the fold
    255 sum T_{j-1} a_j              over the pixel's AMBIGUOUS fragments: fp64 power within ETA of the cut, or depth within
                                     DEPTH_TOL of the stored depth (either side of the 24-bit rounding under GS_DEST_DEPTH_UNORM24)
The first three come to 0.5 + 0.018 + 0.0255 (chunks + 1): 0.57 at two chunks, 1.36 at 32.  tests/test_deep_ref.py prints the
largest any tested pixel receives.

The chunk table is the sentence of gs_internal.hpp written out - 1024, then 4 x 256, 4 x 512, then 1024 each, index 31 unbounded -
and chunk_of() searches it; tests/test_deep_ref.py holds it to the values the header's static_assert names.
"""
from dataclasses import dataclass, field

import numpy as np

import quadrant_ref as qr
import surface_ref as ref
from surface_ref import CUT, DELTA, DEPTH_TOL, ETA           # (one statement of each: surface_ref's)

TILE, BIN = ref.TILE, ref.BIN
T_EPS = 1e-4                                   # GS_T_EPS: the stop rule's threshold
CHUNKS_MAX = 32
LIST_CAP = 65536                               # GS_DEEP_LIST_CAP
RLEN = 1024                                    # GS_DEEP_RLEN
NON_SATURATING_T = 1e-2                        # a quadrant is non-saturating when some pixel ends with T >= this
SIZES = [1024] + 4 * [256] + 4 * [512] + (CHUNKS_MAX - 10) * [1024]       # the bounded chunks 0 .. 30
BOUNDARIES = [sum(SIZES[:c + 1]) for c in range(len(SIZES))]              # 1024, 1280, .. 2048, 2560, .. 4096, 5120, .. 26624


def chunk_of(k):
    """The chunk survivor k (0-based) belongs to: the first boundary above it, else the unbounded last chunk."""
    for c, b in enumerate(BOUNDARIES):
        if k < b:
            return c
    return CHUNKS_MAX - 1


def chunk_count(s):
    return 0 if s == 0 else chunk_of(s - 1) + 1


def chunk_first(c):
    return 0 if c == 0 else BOUNDARIES[c - 1]


def edges_below(s):
    """The chunk edges inside a list of s survivors (an edge at s itself closes a chunk but starts none)."""
    return [b for b in BOUNDARIES if b < s]


# -- one quadrant -----------------------------------------------------------------------------------------------------------------
@dataclass
class Quad:
    """One live quadrant of one bin: its survivors and, per pixel, the plain composite."""
    bx: int
    by: int
    q: int
    px: np.ndarray                 # int64 [p] the quadrant's pixels inside the frame / strip
    py: np.ndarray
    splats: np.ndarray             # int64 [S] survivors, near -> far (the caller's numbering)
    in_band: int                   # (entry, quadrant) pairs inside quadrant_ref's band
    a: np.ndarray                  # float64 [S, p] alpha of every fragment, 0 where it is not kept
    rgb: np.ndarray                # float64 [S, 3]
    amb: np.ndarray                # bool [S, p] the fragment could go either way
    amb_at: tuple                  # (survivor [r], pixel [r], alpha if kept [r]) of the ambiguous fragments
    rejected: dict                 # {survivor: alpha [p] it would have without the depth test} where the depth test rejects some of it
    Tb: np.ndarray = field(default=None)     # float64 [S + 1, p]: T before survivor k; row S = the final T (run(); release() drops it)

    @property
    def S(self):
        return int(self.splats.shape[0])

    @property
    def chunks(self):
        return chunk_count(self.S)

    def run(self):
        if self.Tb is None:
            p = self.px.shape[0]
            self.Tb = np.vstack([np.ones((1, p)), np.cumprod(1.0 - self.a, axis=0)]) if self.S else np.ones((1, p))
        return self

    def release(self):
        self.Tb = None

    def dead(self, k):
        """Survivor k contributes at no pixel (the depth test rejects every fragment the fragment rule keeps)."""
        return not self.a[k].any()

    def C_at(self, k):
        """rgb composited by the first k survivors: float64 [p, 3]."""
        self.run()
        return (self.Tb[:k] * self.a[:k]).T @ self.rgb[:k] if k else np.zeros((self.px.shape[0], 3))

    def T_at(self, k):
        return self.run().Tb[k]

    def value(self):
        """(C [p, 3], T [p]) of the whole list."""
        return self.C_at(self.S), self.T_at(self.S)

    def T_after_edges(self):
        """{edge: T [p] after the first `edge` survivors} for every chunk edge inside the list."""
        return {b: self.T_at(b) for b in edges_below(self.S)}

    def non_saturating(self):
        return float(self.T_at(self.S).max(initial=0.0)) >= NON_SATURATING_T if self.px.shape[0] else True

    def saturation_point(self, eps=T_EPS / 4):
        """The first survivor count at which every pixel holds T <= eps (None: never)."""
        self.run()
        done = np.nonzero(self.Tb.max(axis=1) <= eps)[0]
        return int(done[0]) if done.size else None

    def slack(self):
        """255 sum T_{j-1} a_j over the ambiguous fragments: float64 [p], in 1/255."""
        out = np.zeros(self.px.shape[0])
        k, i, alpha = self.amb_at
        if k.shape[0]:
            np.add.at(out, i, 255.0 * self.run().Tb[k, i] * alpha)
        return out

    def tolerance(self, chunks=None):
        """Per pixel, in 1/255 (see the module's docstring).  `chunks`: the chunks the executor merges (default: the table's)."""
        chunks = self.chunks if chunks is None else chunks
        return 0.5 + 255.0 * DELTA + 255.0 * T_EPS * (chunks + 1) + self.slack()

    # -- the list edited: what a wrong kernel would composite ------------------------------------------------------------------
    def of_list(self, idx):
        """(C, T) of the survivors `idx` (any order, repeats allowed) composited from T = 1."""
        p = self.px.shape[0]
        if len(idx) == 0:
            return np.zeros((p, 3)), np.ones(p)
        a = self.a[np.asarray(idx, np.int64)]
        t = np.vstack([np.ones((1, p)), np.cumprod(1.0 - a, axis=0)])
        return (t[:-1] * a).T @ self.rgb[np.asarray(idx, np.int64)], t[-1]

    def edited(self, edits):
        """(C, T) of the list with `edits` applied: [(lo, hi, replacement survivor indexes)] - sorted, disjoint.  The stretches
        between the edits are taken from the unedited walk: segment [x, y) = ((C(y) - C(x)) / T(x), T(y) / T(x))."""
        self.run()
        p = self.px.shape[0]
        C, T = np.zeros((p, 3)), np.ones(p)

        def over(Cs, Ts):
            nonlocal C, T
            C = C + T[:, None] * Cs
            T = T * Ts
        at = 0
        for lo, hi, rep in list(edits) + [(self.S, self.S, [])]:
            assert at <= lo <= hi <= self.S
            if lo > at:
                Cs, Ts = self.of_list(np.arange(at, lo)) if lo - at <= 4096 else self._stretch(at, lo)
                over(Cs, Ts)
            over(*self.of_list(rep))
            at = hi
        return C, T

    def _stretch(self, x, y):
        Tx = self.T_at(x)
        safe = np.where(Tx > 0, Tx, 1.0)
        C = np.where((Tx > 0)[:, None], (self.C_at(y) - self.C_at(x)) / safe[:, None], 0.0)
        T = np.where(Tx > 0, self.T_at(y) / safe, 0.0)
        if (Tx <= 1e-12).any():                            # (too little left to divide by: walk it)
            return self.of_list(np.arange(x, y))
        return C, T

    def mutations(self, b):
        """The mutations of interest at the chunk edge b (survivors b - 1 | b), each as (name, (C, T), the survivors it drops,
        repeats or moves); a mutation whose survivors do not exist in this list is left out.  A mutation that touches a dead()
        survivor changes nothing a frame could show; "re-admit" is there for those: the survivor composited as if its depth passed."""
        S, out = self.S, []
        if b - 1 < S and b >= 1:
            out.append(("drop b-1", self.edited([(b - 1, b, [])]), [b - 1]))
        if b < S:
            out.append(("drop b", self.edited([(b, b + 1, [])]), [b]))
            out.append(("duplicate b", self.edited([(b, b + 1, [b, b])]), [b]))
            out.append(("swap b-1, b", self.edited([(b - 1, b + 1, [b, b - 1])]), [b - 1, b]))
            # chunk c = chunk_of(b) starts at b + 1 and keeps its length: it misses b and takes the first survivor of the chunk
            # behind it, which that chunk composites again
            c = chunk_of(b)
            end = BOUNDARIES[c] if c < len(BOUNDARIES) else S
            late = [(b, b + 1, [])] + ([(end, end + 1, [end, end])] if c < len(BOUNDARIES) and end < S else [])
            out.append(("chunk starts late", self.edited(late), [b]))
        for k in (b - 1, b):
            if 0 <= k < S and k in self.rejected and self.dead(k):
                row = self.a[k].copy()
                self.a[k] = self.rejected[k]
                out.append((f"re-admit hidden {'b-1' if k == b - 1 else 'b'}", self.edited([(k, k + 1, [k])]), []))
                self.a[k] = row
        if self.chunks >= 2:
            last = chunk_first(self.chunks - 1)
            if float(self.T_at(last).max()) >= NON_SATURATING_T:       # (behind a saturated chunk the fold SHOULD ignore it)
                out.append(("fold ignores the last chunk", (self.C_at(last), self.T_at(last)), []))
            out.append(("fold ignores all behind chunk 0", (self.C_at(BOUNDARIES[0]), self.T_at(BOUNDARIES[0])), []))
        if self.chunks == CHUNKS_MAX and b == BOUNDARIES[-1] + 1024 and b < S:
            out.append(("chunk 31 bounded", (self.C_at(b), self.T_at(b)), []))
        return out


def rgba_of(C, T):
    """What write_pixels forms over the clear colour: rgb = C, alpha = 1 - T; float64 [p, 4] in 1/255."""
    return 255.0 * np.concatenate([np.clip(C, 0.0, 1.0), np.clip(1.0 - T, 0.0, 1.0)[:, None]], axis=1)


# -- a draw -------------------------------------------------------------------------------------------------------------------------
def rec_rgb(recs):
    r = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 8)
    return np.stack([r[:, 6] & 0xFFFF, r[:, 6] >> 16, r[:, 7] & 0xFFFF], axis=1).astype(np.float64) / 65535.0


def live(draw, bx, by, q, rows=None):
    """BinGeom::live of quadrant q of bin (bx, by) for the frame, or the strip of 16-px tile rows `rows`."""
    y0, y1 = qr.live_rows(draw.height, rows)
    qx0, qy0 = bx * BIN + (q & 1) * TILE, by * BIN + (q >> 1) * TILE
    return qx0 < draw.width and qy0 < y1 and qy0 + TILE > y0


def list_of(draw, bx, by):
    """(begin, n) of the entry list of the list bin the 32-px bin (bx, by) lies in."""
    per = draw.list_shift - 1
    lid = ((by >> per) - draw.list_row_begin) * draw.lists_x + (bx >> per)
    b, e = (int(v) for v in draw.ranges[lid])
    return (b, e - b) if e > b else (0, 0)


def _depth_fragments(draw, splats, px, py):
    """(passes bool [m, p], ambiguous bool [m, p]) of the destination's LEQUAL test, either mode."""
    m, p = len(splats), len(px)
    if draw.dest_depth is None:
        return np.ones((m, p), dtype=bool), np.zeros((m, p), dtype=bool)
    d = np.asarray(draw.dest_depth, np.float32)[py, px].astype(np.float64)[None, :]
    z = draw.z[splats][:, None]
    if draw.unorm24:
        f = lambda v: np.floor(v * 16777215.0 + 0.5)
        ok, lo, hi = f(z) <= f(d), f(z - DEPTH_TOL) <= f(d), f(z + DEPTH_TOL) <= f(d)
        return ok, lo != hi
    return z <= d, np.abs(z - d) <= DEPTH_TOL


def quadrant(draw, bx, by, q, rows=None, smap=None):
    """The model of quadrant q of bin (bx, by): None when the quadrant is not live."""
    if not live(draw, bx, by, q, rows):
        return None
    smap = draw.splat_of_slot() if smap is None else smap
    y0, y1 = qr.live_rows(draw.height, rows)
    qx0, qy0 = bx * BIN + (q & 1) * TILE, by * BIN + (q >> 1) * TILE
    ys, xs = np.arange(max(qy0, y0), min(qy0 + TILE, y1)), np.arange(qx0, min(qx0 + TILE, draw.width))
    py, px = (v.ravel() for v in np.meshgrid(ys, xs, indexing="ij"))
    begin, n = list_of(draw, bx, by)
    splats = smap[draw.entries[begin:begin + n]].astype(np.int64)
    assert not (splats == ref.NONE).any(), "a list names a record slot no visible splat owns"
    recs, rects = draw.recs[splats], draw.rects[splats]
    kept = ((qr.kernel_test32(recs, rects, bx, by) >> np.uint32(q)) & 1).astype(bool)
    # the band: among the entries whose rect covers the quadrant's tile, neither surely reaching a pixel nor surely outside the box
    cand = np.nonzero(((qr.quadrant_mask(rects, bx, by) >> np.uint32(q)) & 1).astype(bool))[0]
    box = qr.box_min64(recs[cand], np.full(cand.shape, qx0), np.full(cand.shape, qy0))
    near = cand[~(box > qr.LIMIT + qr.BAND)]
    pw = ref.power64(recs[near], px, py)
    sure = (pw.min(axis=1) < CUT - qr.BAND) if pw.shape[1] else np.zeros(near.shape, dtype=bool)
    in_band = int((~sure).sum())
    sel = np.nonzero(kept)[0]
    pos = np.searchsorted(near, sel)                       # survivors are among `near` unless the test kept a must-drop pair
    known = (pos < near.shape[0]) & (near[np.minimum(pos, max(near.shape[0] - 1, 0))] == sel) if near.shape[0] else np.zeros(sel.shape, bool)
    if known.all():
        pw = pw[pos]
    else:
        in_band += int((~known).sum())
        pw = ref.power64(recs[sel], px, py)
    in_band += int((sure & ~kept[near]).sum())              # a pair that surely reaches a pixel, dropped
    surv = splats[sel]
    ok, damb = _depth_fragments(draw, surv, px, py)
    alpha = ref.alpha64(recs[sel])[:, None] * np.exp2(-pw)
    amb = (ok | damb) & (np.abs(pw - CUT) <= ETA) | damb & (pw < CUT + ETA)
    keep = ok & (pw < CUT)
    ak, ai = np.nonzero(amb)
    free = np.where(pw < CUT, alpha, 0.0)
    rejected = {int(k): free[k] for k in np.nonzero((~ok & (pw < CUT)).any(axis=1))[0]}
    return Quad(bx, by, q, px, py, surv, in_band, np.where(keep, alpha, 0.0), rec_rgb(recs[sel]), amb, (ak, ai, alpha[ak, ai]), rejected)


def bins_with_lists(draw, rows=None):
    """The 32-px bins of the frame / strip whose list is not empty: [(bx, by)]."""
    y0, y1 = qr.live_rows(draw.height, rows)
    out = []
    for by in range(y0 // BIN, (y1 + BIN - 1) // BIN):
        for bx in range((draw.width + BIN - 1) // BIN):
            if list_of(draw, bx, by)[1]:
                out.append((bx, by))
    return out


# -- the comparison the GPU tests and the CPU proof share --------------------------------------------------------------------------
def compare_quadrant(frame_rows, row0, quad, chunks=None, what=""):
    """The RGBA8 pixels of `frame_rows` (row 0 = pixel row `row0`) against the model of one quadrant.  Returns (complaints, worst
    error over tolerance, largest tolerance)."""
    if quad.px.shape[0] == 0:
        return [], 0.0, 0.0
    return compare_values(frame_rows[quad.py - row0, quad.px].astype(np.float64), quad, chunks, what)


def compare_values(got255, quad, chunks=None, what=""):
    """got255: float [p, 4] channel values in 1/255 (a frame's bytes, or a mutated model's unrounded values)."""
    want = rgba_of(*quad.value())
    tol = quad.tolerance(chunks)
    err = np.abs(got255 - want).max(axis=1)
    bad = np.nonzero(err > tol)[0]
    out = []
    if bad.size:
        i = bad[np.argmax(err[bad] - tol[bad])]
        out.append(f"{what} bin ({quad.bx}, {quad.by}) quadrant {quad.q} (S = {quad.S}): {bad.size} pixels beyond the tolerance, worst "
                   f"({int(quad.px[i])}, {int(quad.py[i])}) got {np.round(got255[i], 2).tolist()} model {np.round(want[i], 3).tolist()} "
                   f"tolerance {tol[i]:.3f}")
    return out, float((err / tol).max()), float(tol.max())


# -- integer predictions -------------------------------------------------------------------------------------------------------------
def predicted_closed(quads):
    """Chunk partials the per-bin kernel closes: (low, high, quadrants exactly on an edge).  A list that ends exactly on an edge
    may or may not close its last chunk - the header's definition is indifferent, the fold of {C, T} with an empty chunk (0, 1) is
    exact - so the prediction is the pair {low, high}; the kernel must choose the same way in every such quadrant."""
    low = sum(max(q.chunks - 1, 0) for q in quads)
    on_edge = [q for q in quads if q.S in BOUNDARIES]
    return low, low + len(on_edge), on_edge


def walk_bounds(quad, deep):
    """[low, high] (splat, quadrant) pairs an executor composites in this quadrant, from the definition alone.  A chunk walks its
    survivors until a saturation test (every 8th survivor of the chunk) finds every pixel's CHUNK-LOCAL T <= 1e-4.  In fp64 the
    kernel's fp32 T cannot be told from the threshold within a factor of 4 either way at the depths tested here (an fp32 product
    of thousands of factors drifts by ~1e-3 relative; the factor is generous), so a chunk has surely not stopped while the model's
    local T is above 4e-4 somewhere and has surely stopped at the first test after it is below 1e-4 / 4 everywhere.
      deep = False  the per-bin kernel: chunk after chunk, ending with the first chunk that stops (or leaves the folded T <= 1e-4);
      deep = True   the deep pass: every chunk is walked on its own, whatever the chunks in front of it did.
    A non-saturating quadrant gets [S, S]."""
    if quad.S == 0:
        return 0, 0
    lo = hi = 0
    for c in range(quad.chunks):
        first = chunk_first(c)
        end = min(BOUNDARIES[c], quad.S) if c < len(BOUNDARIES) else quad.S
        local = np.cumprod(1.0 - quad.a[first:end], axis=0).max(axis=1)
        may_have_stopped = np.nonzero(local <= 4.0 * T_EPS)[0]
        surely_shut = np.nonzero(local <= T_EPS / 4.0)[0]
        n = end - first
        k_lo = min(n, int(may_have_stopped[0]) + 1) if may_have_stopped.size else n
        k_hi = min(n, (int(surely_shut[0]) + 1 + 7) // 8 * 8) if surely_shut.size else n
        lo, hi = lo + k_lo, hi + k_hi
        if not deep:
            folded = quad.T_at(end).max()
            if surely_shut.size or folded <= T_EPS / 4.0:
                break                                      # the walk surely ends here ...
            if may_have_stopped.size or folded <= 4.0 * T_EPS:
                return lo, quad.S                          # ... or may end here: anything up to the whole list is possible
    return lo, hi
