"""Host model (numpy, fp64) of the two shapes of k_tile_blend_rop8 (GS_DRAW_ROP8, GS_DRAW_ROP8_FULL) and of k_rop8_window
(csrc/tile_blend.hip): the reference's RGBA8 render target - back to front, every channel rounded to 8 bits after EVERY splat.

The rounding is discontinuous, so the kernels cannot be held to a tolerance.  They are held to an INTERVAL per pixel and channel.
One step of the target is  c' = q8(clamp((1 - a) c + a s)),  q8(v) = floor(255 v + 0.5) / 255.  It is monotone in c ((1 - a) >= 0)
and, for fixed c and s, linear in a - so its extremes over a range of alphas lie at the range's ends.  The model carries [lo, hi]
(integers, in 1/255) through a quadrant's survivors far -> near:  lo takes the smaller of the two ends of the alpha range applied
to lo, hi the larger applied to hi.  The alpha range of a fragment is a (1 -+ DELTA) around the fp64 alpha - surface_ref's measured
bound on ONE fragment's fp32 alpha, v_exp_f32 included; an AMBIGUOUS fragment (power within ETA of the cut, depth within DEPTH_TOL
of the stored depth) has the hull of "kept" and "alpha 0".  The interval is sound (the device's value lies in it whatever its
alphas are inside their ranges) and sharp: tests/test_rop8_ref.py measures it on random lists - never wider than 1 step, the colour
channels pinned to a single byte on 96 % and more of the values at every depth and loudness, and the alpha channel alike except
under long faint lists: alpha only ever rises and STALLS once a (255 - alpha) < 0.5 (the kernel's own comment), and lo and hi may
stall on neighbouring bytes that nothing merges again - and >= 95 % of all values on every designed case.

PAD - how far the device's fp32 evaluation of one step can sit from the exact value of the same step, in 1/255, one rounding per
operation (half an ulp: 2^-24 relative).  composite_rop8 / q8_pair_fused:
    c held as k * (1/255):   1/255 rounded to fp32 and the product rounded: 2 roundings of a value <= 1      255 x 2^-23 = 3.04e-5
    om = 1 - a               one rounding of a value <= 1 (half an ulp below 1: 2^-25), times c <= 1          255 x 2^-25 = 0.76e-5
    a * src                  src = u16 * (1/65535) (2 roundings), the product (1): a src <= 1                 255 x 3 x 2^-24 = 4.56e-5
    v_pk_fma_f32 .. clamp    om c + (a src), rounded once, v <= 1                                              255 x 2^-24 = 1.52e-5
    fma(v, 255, 0.5)         rounded once, a value < 256 (half an ulp in [128, 256): 2^-17)                    2^-17       = 0.76e-5
    floor, * (1/255)         floor is exact; the product is the first line's
which sum to PAD = 1.064e-4 steps.  It is added to both ends before the floor at every step.  (The relative error of the ALPHA is
not in PAD: it is the range a (1 -+ DELTA).)  k_rop8_window and the CPU oracle evaluate the step unfused - a * s and om * c rounded
apart, v * 255 and + 0.5 rounded apart: one more rounding of each kind, PAD_UNFUSED = PAD + 255 x 2^-24 + 2^-17 = 1.29e-4.  (The CPU
oracle takes its source colour as byte / 255 and the record holds unorm16(byte) = 257 byte: the same number, byte / 255 = 257 byte /
65535, up to the one fp32 rounding PAD counts.)

The bounded walk (GS_DRAW_ROP8).  Pass 1, front to back: T per pixel over the quadrant's survivors, a fragment counting only from
alpha >= 1/64, tested after every 8th survivor OF THE LIST (the cadence counter spans the batches), stopping when every pixel of
the quadrant holds T <= 1e-6.  T is an fp32 product on the device, so the model keeps the SET of candidate stop counts: the walk
has surely stopped at the first test where the model's largest possible T is <= 1e-6 / 4 everywhere, and may stop from the first
test where the smallest possible T is <= 4e-6 everywhere ("possible": alphas anywhere in a (1 -+ DELTA), those within DELTA of 1/64
counted or not, ambiguous fragments kept or not).  The factor 4 is deep_ref.walk_bounds': one factor (1 - a) has the relative error
a DELTA / (1 - a) + 2^-24 - below 6.1e-4 while a <= 0.895, the loudest fragment the designed stacks put on the pixel that decides
(the quadrant's far corner) - and the lists tested here hold <= 1100 survivors of which a few tens are that loud and the rest have
a <= 0.16 (1.4e-5 each): the product drifts by less than 5 %, far inside the factor.  Pass 2 composites the first k survivors back to
front; the pixel interval is the hull over the candidates k.

Integer predictions per blend bin (gs_mesh_debug_read what = 4):  pairs = the sum of the stop counts over the live quadrants (S_q
for the full walk), entries scanned = n for the full walk and min(256 (last + 1), n) for the bounded one, `last` the farthest
batch any live quadrant's pass 1 reached.  Exact where every quadrant has one candidate, else a closed range.

mutations(): what a wrong kernel would leave - exact bytes from the same arithmetic with every alpha at its fp64 centre - one per
candidate fault in the batch / group / stop logic.  tests/test_rop8_ref.py proves that the comparison used on the device rejects
each of them."""
from dataclasses import dataclass, field

import numpy as np

import deep_ref
from surface_ref import DELTA

BATCH, GROUP, CHECK = 256, 64, 8               # BLEND_THREADS, the wave, GS_BLEND_CHECK
T_EPS = 1e-6                                   # GS_ROP8_T_EPS
A_MIN = 1.0 / 64.0                             # GS_ROP8_A_MIN
FACTOR = 4.0                                   # deep_ref.walk_bounds' factor between the model's T and the device's
PAD = 255.0 * (2.0 ** -23 + 2.0 ** -25 + 3.0 * 2.0 ** -24 + 2.0 ** -24) + 2.0 ** -17
PAD_UNFUSED = PAD + 255.0 * 2.0 ** -24 + 2.0 ** -17
FULL, BOUNDED = "full", "bounded"


# -- the arithmetic -----------------------------------------------------------------------------------------------------------------
def q8(v):
    return np.floor(np.clip(v, 0.0, 255.0) + 0.5)


def walk_interval(alo, ahi, src, lo, hi, pad=PAD):
    """[lo, hi] after the fragments alo / ahi [S, p] (the two ends of each alpha range), sources src [S, 4] in 1/255, applied far
    -> near, i.e. from row S - 1 to row 0, to the start lo, hi float [p, 4] (integers)."""
    lo, hi = lo.copy(), hi.copy()
    for j in range(alo.shape[0] - 1, -1, -1):
        a0, a1 = alo[j][:, None], ahi[j][:, None]
        if not a1.any():
            continue
        s = src[j][None, :]
        lo = q8(np.minimum(lo + a0 * (s - lo), lo + a1 * (s - lo)) - pad)
        hi = q8(np.maximum(hi + a0 * (s - hi), hi + a1 * (s - hi)) + pad)
    return lo, hi


def walk_exact(a, src, start, alpha_unrounded=False):
    """The bytes [p, 4] the arithmetic gives with the alphas a [S, p] exactly: rows S - 1 .. 0 over `start`."""
    c = start.astype(np.float64).copy()
    for j in range(a.shape[0] - 1, -1, -1):
        aj = a[j][:, None]
        v = c + aj * (src[j][None, :] - c)
        c = q8(v)
        if alpha_unrounded:
            c[:, 3] = np.clip(v[:, 3], 0.0, 255.0)
    return q8(c)


# -- one quadrant ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Model:
    quad: object                   # deep_ref.Quad
    mode: str
    start: np.ndarray              # float [p, 4]: the destination's bytes, or 0
    pos: np.ndarray                # int64 [S]: list position of every survivor
    n: int                         # entries of the bin's list
    stops: list                    # candidate (survivors composited, last batch pass 1 looked at)
    lo: np.ndarray = None          # float [p, 4] integers
    hi: np.ndarray = None
    src: np.ndarray = field(default=None, repr=False)

    @property
    def S(self):
        return self.quad.S

    @property
    def batches(self):
        return (self.n + BATCH - 1) // BATCH

    @property
    def unique(self):
        return len(self.stops) == 1

    def pinned(self):
        return self.lo == self.hi


def alpha_ranges(quad, delta=DELTA):
    """(alo, ahi, centre-if-kept) [S, p]: an ambiguous fragment ranges from 0 to its alpha-if-kept."""
    a = quad.a
    kept = a.copy()
    k, i, alpha = quad.amb_at
    if k.shape[0]:
        kept[k, i] = alpha
    alo = np.where(quad.amb, 0.0, a * (1.0 - delta))
    ahi = np.minimum(np.where(quad.amb, kept, a) * (1.0 + delta), 1.0)
    return alo, ahi, kept


def sources(quad):
    return 255.0 * np.concatenate([quad.rgb, np.ones((quad.S, 1))], axis=1)


def pass1(quad, n, pos, delta=DELTA, factor=FACTOR, restart_per_batch=False, a_min=A_MIN, exact=False):
    """Candidate (stop count, last batch) of the bounded walk's pass 1.  exact: alphas at their centre and the threshold as it is -
    one candidate (what mutations() walks).  restart_per_batch: the cadence counter reset at every batch (a mutation)."""
    S, batches = quad.S, (n + BATCH - 1) // BATCH
    never = (S, max(batches - 1, 0))
    if S == 0 or quad.px.shape[0] == 0:
        return [never]
    alo, ahi, kept = alpha_ranges(quad, 0.0 if exact else delta)
    if exact:
        t_small = t_large = np.cumprod(1.0 - np.where(quad.a >= a_min, quad.a, 0.0), axis=0).max(axis=1)
        may_eps = sure_eps = T_EPS
    else:
        t_small = np.cumprod(1.0 - np.where(ahi >= a_min, ahi, 0.0), axis=0).max(axis=1)
        t_large = np.cumprod(1.0 - np.where(alo >= a_min, alo, 0.0), axis=0).max(axis=1)
        may_eps, sure_eps = factor * T_EPS, T_EPS / factor
    if restart_per_batch:
        b = pos // BATCH
        in_batch = np.arange(S) - np.searchsorted(b, b, side="left")          # rank of the survivor inside its batch
        tests = np.nonzero((in_batch + 1) % CHECK == 0)[0] + 1
    else:
        tests = np.arange(CHECK, S + 1, CHECK)
    out = []
    for k in tests:
        if t_small[k - 1] <= may_eps:
            out.append((int(k), int(pos[k - 1] // BATCH)))
            if t_large[k - 1] <= sure_eps:
                break
    else:
        out.append(never)
    return sorted(set(out))


def survivor_positions(draw, quad, smap=None):
    smap = draw.splat_of_slot() if smap is None else smap
    begin, n = deep_ref.list_of(draw, quad.bx, quad.by)
    listed = smap[draw.entries[begin:begin + n]].astype(np.int64)
    pos = np.nonzero(np.isin(listed, quad.splats))[0]
    # (a splat is listed once per list; the survivors are a subsequence of the list)
    assert pos.shape[0] == quad.S and np.array_equal(listed[pos], quad.splats)
    return pos, n


def start_of(quad, dest_rgba):
    if dest_rgba is None:
        return np.zeros((quad.px.shape[0], 4))
    return np.asarray(dest_rgba)[quad.py, quad.px].astype(np.float64)


def model(draw, bx, by, q, mode, dest_rgba=None, rows=None, smap=None, pad=PAD):
    """The model of quadrant q of bin (bx, by) for a draw in `mode`: None when the quadrant is not live.  dest_rgba: uint8 [H, W, 4]
    of the whole frame (the destination's colour plane) or None - the cleared target."""
    quad = deep_ref.quadrant(draw, bx, by, q, rows, smap)
    if quad is None:
        return None
    pos, n = survivor_positions(draw, quad, smap)
    start = start_of(quad, dest_rgba)
    stops = pass1(quad, n, pos) if mode == BOUNDED else [(quad.S, max((n + BATCH - 1) // BATCH - 1, 0))]
    m = Model(quad, mode, start, pos, n, stops, src=sources(quad))
    alo, ahi, _ = alpha_ranges(quad)
    for k in sorted({k for k, _ in stops}):
        lo, hi = walk_interval(alo[:k], ahi[:k], m.src[:k], start, start, pad)
        m.lo = lo if m.lo is None else np.minimum(m.lo, lo)
        m.hi = hi if m.hi is None else np.maximum(m.hi, hi)
    return m


def models_of(draw, mode, dest_rgba=None, rows=None, **kw):
    """{(bx, by, q): Model} of every live quadrant of every bin with a list."""
    smap = draw.splat_of_slot()
    out = {}
    for bx, by in deep_ref.bins_with_lists(draw, rows):
        for q in range(4):
            m = model(draw, bx, by, q, mode, dest_rgba, rows, smap, **kw)
            if m is not None:
                out[(bx, by, q)] = m
    return out


# -- integer predictions --------------------------------------------------------------------------------------------------------------
def walked_range(draw, mode, rows=None):
    """[low, high] (splat, quadrant) pairs a whole draw in `mode` composites (RenderStats.splats_walked), without the pixel
    intervals: the sum of S_q for the full walk, of the stop candidates for the bounded one; a pair inside quadrant_ref's band (the
    quadrant test may keep it or not) widens the range by one either way.  low == high: the prediction is exact."""
    smap = draw.splat_of_slot()
    lo = hi = 0
    for bx, by in deep_ref.bins_with_lists(draw, rows):
        for q in range(4):
            quad = deep_ref.quadrant(draw, bx, by, q, rows, smap)
            if quad is None:
                continue
            ks = [quad.S]
            if mode == BOUNDED:
                pos, n = survivor_positions(draw, quad, smap)
                ks = [k for k, _ in pass1(quad, n, pos)]
            lo, hi = lo + min(ks) - quad.in_band, hi + max(ks) + quad.in_band
    return lo, hi


def predictions(M):
    """{(bx, by): ((pairs low, high), (entries low, high))} from the models of a draw."""
    out = {}
    for (bx, by, q), m in M.items():
        ks, ls = [k for k, _ in m.stops], [l for _, l in m.stops]
        (p0, p1), (l0, l1), n = out.get((bx, by), ((0, 0), (0, 0), m.n))
        out[(bx, by)] = ((p0 + min(ks), p1 + max(ks)), (max(l0, min(ls)), max(l1, max(ls))), n)
    scanned = lambda last, n, mode: n if mode == FULL else min(BATCH * (last + 1), n)
    mode = next(iter(M.values())).mode if M else FULL
    return {b: (p, (scanned(l[0], n, mode), scanned(l[1], n, mode))) for b, (p, l, n) in out.items()}


def check_integers(stats, M, what=""):
    """stats: {(bx, by): (entries scanned, pairs)} of the draw; every bin of it.  Returns complaints."""
    want = predictions(M)
    bad = []
    for b in sorted(set(stats) | set(want)):
        got_e, got_p = stats.get(b, (0, 0))
        (p0, p1), (e0, e1) = want.get(b, ((0, 0), (0, 0)))
        if not (p0 <= got_p <= p1 and e0 <= got_e <= e1):
            bad.append(f"{what} bin {b}: {got_p} pairs / {got_e} entries scanned, the model says {p0} .. {p1} / {e0} .. {e1}")
    return bad


# -- the comparison the GPU tests and the CPU proof share ----------------------------------------------------------------------------
def compare(frame_rows, row0, m, what=""):
    """The RGBA8 pixels of `frame_rows` (row 0 = pixel row `row0`) against the model of one quadrant, every pixel of it.  Returns
    (complaints, the share of pinned channel values, the widest interval in steps)."""
    if m.quad.px.shape[0] == 0:
        return [], 1.0, 0
    return compare_values(np.asarray(frame_rows)[m.quad.py - row0, m.quad.px].astype(np.float64), m, what)


def compare_values(got, m, what=""):
    bad = (got < m.lo) | (got > m.hi)
    out = []
    if bad.any():
        i, ch = (int(v[0]) for v in np.nonzero(bad))
        out.append(f"{what} bin ({m.quad.bx}, {m.quad.by}) quadrant {m.quad.q} ({m.mode}, S = {m.S}, stops {m.stops}): {int(bad.sum())} "
                   f"values outside the interval, first pixel ({int(m.quad.px[i])}, {int(m.quad.py[i])}) channel {ch}: got "
                   f"{got[i].tolist()}, interval {m.lo[i].tolist()} .. {m.hi[i].tolist()}")
    return out, float(m.pinned().mean()), int((m.hi - m.lo).max())


def check_frame(frame, M, row0=0, dest_rgba=None, what=""):
    """A frame (or strip) against the models of its draw, every pixel: inside the interval where a quadrant is modelled, the
    destination's byte (or clear) everywhere else.  Returns (complaints, pinned share over all modelled values, widest interval)."""
    frame = np.asarray(frame)
    bad, pinned, total, widest = [], 0, 0, 0
    covered = np.zeros(frame.shape[:2], dtype=bool)
    for m in M.values():
        b, share, w = compare(frame, row0, m, what)
        bad += b
        pinned, total, widest = pinned + int(m.pinned().sum()), total + m.lo.size, max(widest, w)
        covered[m.quad.py - row0, m.quad.px] = True
    rest = np.zeros_like(frame) if dest_rgba is None else np.asarray(dest_rgba)[row0:row0 + frame.shape[0]]
    stray = ~covered & (frame != rest).any(axis=-1)
    if stray.any():
        y, x = (int(v[0]) for v in np.nonzero(stray))
        bad.append(f"{what}: {int(stray.sum())} pixels outside every list differ from the target's start, first ({x}, {y + row0}) = "
                   f"{frame[y, x].tolist()}")
    return bad, (pinned / total if total else 1.0), widest


# -- what a wrong kernel would produce ---------------------------------------------------------------------------------------------------
@dataclass
class Mutant:
    name: str
    q: int                         # the quadrant whose walk it changes
    bytes: dict                    # {q: float [p, 4]} of the quadrants it changes (the others keep the model's centre walk)
    pairs: int                     # pairs the bin's walk composites under it
    scanned: int                   # entries it scans
    changes_walk: bool             # it composites another number of pairs or scans another number of entries


def _seq_bytes(m, seq, start=None, a=None, **kw):
    a = m.quad.a if a is None else a
    idx = np.asarray(seq, np.int64)[::-1] if len(seq) else np.zeros(0, np.int64)      # walk_exact applies the LAST row first
    return walk_exact(a[idx], m.src[idx], m.start if start is None else start, **kw)


def centre(m):
    """(stop count, last batch, bytes) of the walk with every alpha at its centre."""
    k, last = (pass1(m.quad, m.n, m.pos, exact=True)[0] if m.mode == BOUNDED else m.stops[0])
    return k, last, _seq_bytes(m, list(range(k - 1, -1, -1)))


def kernel_order(m, k, ascending_in_group=False):
    """The order in which the kernel composites the first k survivors: batches from the farthest, groups of 64 list entries from
    the farthest, a group's survivors descending (or, mutated, ascending)."""
    idx = np.arange(k)
    key_group = m.pos[:k] // GROUP
    order = sorted(idx.tolist(), key=lambda j: (-int(key_group[j]), j if ascending_in_group else -j))
    return order


def mutations(Mbin, edges=None):
    """Mbin: {q: Model} of ONE bin (every live quadrant of it, one mode); edges: {q: [list positions e]} - the targeted batch /
    group edges (entries e - 1 | e both survivors of q).  Returns [Mutant]."""
    mode = next(iter(Mbin.values())).mode
    base = {q: centre(m) for q, m in Mbin.items()}
    n = next(iter(Mbin.values())).n
    scan = lambda last: n if mode == FULL else min(BATCH * (last + 1), n)
    pairs0 = sum(k for k, _, _ in base.values())
    scanned0 = scan(max(l for _, l, _ in base.values()))
    out = []

    def add(name, changed, stops=None):
        """changed: {q: bytes}; stops: {q: (k, last)} where the walk differs."""
        ks = {q: (base[q][0], base[q][1]) for q in Mbin}
        ks.update(stops or {})
        pairs, scanned = sum(k for k, _ in ks.values()), scan(max(l for _, l in ks.values()))
        out.append(Mutant(name, next(iter(changed)), changed, pairs, scanned, (pairs, scanned) != (pairs0, scanned0)))

    for q, m in Mbin.items():
        k, last, _ = base[q]
        desc = list(range(k - 1, -1, -1))
        where = {int(p): j for j, p in enumerate(m.pos)}
        for e in (edges or {}).get(q, []):
            kind = "batch" if e % BATCH == 0 else "group"
            jb, ja = where[e - 1], where[e]                              # survivors on the near / far side of the edge
            if ja >= k:
                continue                                                 # (the bounded walk ends in front of this edge)
            at = lambda seq, j: seq.index(j)
            s = desc.copy(); s.pop(at(s, jb)); add(f"drop {kind} edge - 1", {q: _seq_bytes(m, s)}, {q: (k - 1, last)})
            s = desc.copy(); s.pop(at(s, ja)); add(f"drop {kind} edge", {q: _seq_bytes(m, s)}, {q: (k - 1, last)})
            s = desc.copy(); s.insert(at(s, ja), ja); add(f"duplicate {kind} edge", {q: _seq_bytes(m, s)}, {q: (k + 1, last)})
            s = desc.copy(); i0, i1 = at(s, ja), at(s, jb); s[i0], s[i1] = s[i1], s[i0]; add(f"swap {kind} edge", {q: _seq_bytes(m, s)})
        if m.S:
            add("survivors ascending inside a group", {q: _seq_bytes(m, kernel_order(m, k, True))})
        r = n - BATCH * (m.batches - 1) if m.batches else 0
        if m.batches >= 2 and r < BATCH:                                 # the partial batch taken as the NEAREST: batch 0 holds r
            keep = [j for j in desc if not (r <= m.pos[j] < BATCH)]      # entries, the 256 - r behind them are never looked at
            add("partial batch nearest", {q: _seq_bytes(m, keep)}, {q: (len(keep), last)})
        if m.start.any():
            add("start from 0", {q: _seq_bytes(m, desc, start=np.zeros_like(m.start))})
        if m.S:
            add("alpha unrounded", {q: _seq_bytes(m, desc, alpha_unrounded=True)})
        for j, free in m.quad.rejected.items():
            if j < k and m.quad.dead(j):
                a = m.quad.a.copy()
                a[j] = free
                add("re-admit a depth-rejected fragment", {q: _seq_bytes(m, desc, a=a)})
                break
        if mode == BOUNDED:
            if k < m.S:
                first = int(np.searchsorted(m.pos, BATCH * last))                       # survivors in front of batch b_stop
                end = int(np.searchsorted(m.pos, BATCH * (last + 1)))
                for d in (-8, -1, 1, 8):
                    kk = min(max(k + d, first), end)
                    if kk != k:
                        add(f"c_stop {d:+d}", {q: _seq_bytes(m, list(range(kk - 1, -1, -1)))}, {q: (kk, last)})
                keep = [j for j in desc if m.pos[j] // BATCH != last]
                add("skip the b_stop batch", {q: _seq_bytes(m, keep)}, {q: (len(keep), last)})
            k2, l2 = pass1(m.quad, n, m.pos, exact=True, restart_per_batch=True)[0]
            if (k2, l2) != (k, last):
                add("cadence restarts at every batch", {q: _seq_bytes(m, list(range(k2 - 1, -1, -1)))}, {q: (k2, l2)})
            k3, l3 = pass1(m.quad, n, m.pos, exact=True, a_min=0.0)[0]
            if (k3, l3) != (k, last):
                add("1/64 rule ignored", {q: _seq_bytes(m, list(range(k3 - 1, -1, -1)))}, {q: (k3, l3)})
            if q != 0 and 0 in Mbin:                                     # every wave takes wave 0's (b_stop, c_stop)
                k0, l0, _ = base[0]
                m0 = Mbin[0]
                if k0 < m0.S:
                    c0 = k0 - int(np.searchsorted(m0.pos, BATCH * l0))
                    mine = int(np.searchsorted(m.pos, BATCH * l0))
                    kk = min(mine + c0, int(np.searchsorted(m.pos, BATCH * (l0 + 1))))
                    if kk != k:
                        add("every wave takes wave 0's stop", {q: _seq_bytes(m, list(range(kk - 1, -1, -1)))}, {q: (kk, l0)})
    return out


def caught(mut, Mbin, stats_model):
    """(a pixel of the bin leaves its interval, an integer prediction breaks) for one mutant: the GPU tests' own comparisons, the
    mutant's bytes standing in for the frame.  stats_model: predictions(...)[bin]."""
    pixel = any(compare_values(b, Mbin[q])[0] for q, b in mut.bytes.items())
    (p0, p1), (e0, e1) = stats_model
    return pixel, not (p0 <= mut.pairs <= p1 and e0 <= mut.scanned <= e1)


# -- the tightness of the interval on random lists ---------------------------------------------------------------------------------------
def simulate(rng, S, peak, falloff, pixels=64, delta=DELTA, pad=PAD):
    """(pinned share of the colour channels, of the alpha channel, widest interval, the centre walk inside) for one random list of S survivors over `pixels` pixels: alphas
    uniform in [0, peak), or - falloff - peak * 2^-power with the power uniform in [0, 5.77)."""
    a = rng.uniform(0.0, peak, size=(S, pixels)) if not falloff else peak * np.exp2(-rng.uniform(0.0, 5.77, size=(S, pixels)))
    src = np.concatenate([np.floor(rng.uniform(0, 65536, size=(S, 3))) / 65535.0 * 255.0, np.full((S, 1), 255.0)], axis=1)
    start = np.zeros((pixels, 4))
    lo, hi = walk_interval(a * (1.0 - delta), a * (1.0 + delta), src, start, start, pad)
    mid = walk_exact(a, src, start)
    pinned = lo == hi
    return float(pinned[:, :3].mean()), float(pinned[:, 3].mean()), int((hi - lo).max()), bool(((mid >= lo) & (mid <= hi)).all())
