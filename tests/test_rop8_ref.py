"""No GPU: the interval model of the ROP8 draw modes (tests/rop8_ref.py) on the designed scenes (tests/rop8_cases.py), from records
of the CPU oracle's vertex stage and the binner's host model - the proof that tests/test_gpu_rop8_edges.py can see something.

Per case: the named list lengths, survivor counts and stop counts are what the host model produces, every quadrant of a targeted
bin has ONE stop candidate, the marker pixels hold no ambiguous fragment, no pair lies in quadrant_ref's band; >= 95 % of the
checked channel values are pinned to a single byte (printed, per case and mode, with the widest interval); the repository's
ROP-emulating oracle lies inside the full walk's interval on every pixel; and every mutation of rop8_ref.mutations() is rejected
by the comparisons the GPU tests use - a pixel outside its interval, and a broken integer prediction where the mutation changes
the walk - in a case that names it (rop8_cases.CATCHES).  The mutations whose names begin with rop8_cases.ONLY_COUNTERS change only
what lies behind T <= 1e-6: invisible in the colour by design, they must break an integer prediction.

The random-list simulation of the interval's tightness is re-asserted with its figures printed: lists of 64 .. 3000 survivors,
uniform and Gaussian-falloff alphas up to 0.99 / 0.3 / 0.05 - never wider than 1 step, >= 97 % of the colour values pinned in every
class, the alpha channel apart (it stalls under long faint lists)."""
import numpy as np
import pytest

import helpers
import oracle
import rop8_cases as cases
import rop8_ref as rr

MODES = [rr.FULL, rr.BOUNDED]
PINNED = 0.95
_models = {}


def models(name, mode, **kw):
    """(case, draw, {(bx, by, q): Model}) - built once per (case, mode), shared, unchanged."""
    key = (name, mode, tuple(sorted(kw.items())))
    if key not in _models:
        c = cases.case(name)
        d = cases.cpu_draw(c)
        _models[key] = (c, d, rr.models_of(d, mode, c.dest_rgba, **kw))
    return _models[key]


def test_pad_is_the_sum_of_the_docstrings_terms():
    assert abs(rr.PAD - 1.064e-4) < 1e-7 and abs(rr.PAD_UNFUSED - 1.29e-4) < 1e-6 and rr.PAD_UNFUSED < 2e-4
    assert rr.A_MIN == 1.0 / 64.0 and 3.0 / 255.0 * (1.0 + rr.DELTA) < rr.A_MIN < 4.0 / 255.0 * (1.0 - rr.DELTA)


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_conditions(name):
    c, d, M = models(name, rr.BOUNDED)
    for (bx, by), want in c.list_len.items():
        assert rr.deep_ref.list_of(d, bx, by)[1] == want, (name, bx, by)
    for (bx, by), per in c.targets.items():
        for q, t in per.items():
            if not rr.deep_ref.live(d, bx, by, q):
                continue
            m = M[(bx, by, q)]
            assert m.S == t.S, (name, bx, by, q, m.S, t.S)
            assert m.unique, (name, bx, by, q, m.stops)
            marks = cases.marker_pixels(c, m.quad)
            assert not (m.quad.amb.any(axis=0) & marks).any(), (name, bx, by, q)
            for e in t.edges:                                # both sides of a targeted edge are survivors of the quadrant
                assert e - 1 in m.pos and e in m.pos, (name, bx, by, q, e)
            if (bx, by, q) in c.stops:
                assert m.stops == [c.stops[(bx, by, q)]], (name, bx, by, q, m.stops, c.stops[(bx, by, q)])
    assert all(m.quad.in_band == 0 for m in M.values()), name
    # what this case is there for
    if name == "lengths":
        assert sorted(rr.deep_ref.list_of(d, *b)[1] for b in c.targets) == sorted(cases.LENGTHS)
        last = sorted((n - 1) % 256 + 1 for n in cases.LENGTHS)
        assert {1, 64, 65, 128, 129, 193, 255, 256} <= set(last)
        assert len(rr.deep_ref.bins_with_lists(d)) == len(cases.LENGTHS)      # every other bin: n = 0
    if name == "survivors":
        pos = {q: M[cases.AT + (q,)].pos for q in range(4)}
        assert pos[3].size == 0 and rr.deep_ref.live(d, *cases.AT, 3)
        assert not ((pos[0] >= 256) & (pos[0] < 512)).any() and (pos[0] < 256).any() and (pos[0] >= 512).any()
        assert np.intersect1d(pos[0], pos[2]).size == 40     # the pairs: one entry, two quadrants
    if name == "edge8":
        assert [rr.deep_ref.live(d, 8, 5, q) for q in range(4)] == [True, False, False, False]
        assert [rr.deep_ref.live(d, 8, 2, q) for q in range(4)] == [True, False, True, False]
        for rows, want in zip(c.strips, ([True, False, False, False], [False, False, True, False])):
            assert [rr.deep_ref.live(d, 8, 2, q, rows) for q in range(4)] == want
            assert rows[0] % 2 == 1 or rows[1] % 2 == 1      # the cut lies on an odd 16-px tile row
    if name in ("stop_before", "stop_group2", "stop_batch_last"):
        m = M[cases.AT + (0,)]
        (k, last), = m.stops
        c_stop = k - int(np.searchsorted(m.pos, 256 * last))
        in_batch = m.pos[(m.pos >= 256 * last) & (m.pos < 256 * (last + 1))] - 256 * last
        before = [int((in_batch < 64 * g).sum()) for g in range(5)]
        assert last == 1 and last < m.batches - 1
        want = {"stop_before": c_stop == before[2] == 128, "stop_group2": before[2] < c_stop < before[3],
                "stop_batch_last": c_stop == before[4] == 256 and m.pos[k - 1] == 511}[name]
        assert want, (name, c_stop, before)
    if name == "still_staged":
        assert all(M[cases.AT + (q,)].stops == [(16, 0)] for q in range(4)) and M[cases.AT + (0,)].batches == 3
    if name == "stop8":
        assert M[cases.AT + (1,)].S % 8 == 0 and M[cases.AT + (2,)].S % 8 == 5 and M[cases.AT + (0,)].stops == [(8, 0)]
    if name == "stop_last_test":
        m = M[cases.AT + (0,)]
        assert m.S % 8 == 0 and m.pos[-1] == m.n - 1
        assert rr.pass1(m.quad, m.n, m.pos, exact=True) == [(m.S, m.batches - 1)]
        T = np.cumprod(1.0 - np.where(m.quad.a >= rr.A_MIN, m.quad.a, 0.0), axis=0).max(axis=1)
        assert T[m.S - 9] > 0.5 and T[m.S - 1] <= rr.T_EPS / rr.FACTOR        # it DOES saturate, at the very last test
    if name == "faint_pile":
        m = M[cases.AT + (0,)]
        a = m.quad.a[:cases.FAINT_PILE]
        assert 0 < a[a > 0].min() and a.max() * (1.0 + rr.DELTA) < rr.A_MIN and (a > 0).all()
        assert rr.pass1(m.quad, m.n, m.pos, exact=True, a_min=0.0) == [(cases.FAINT_PILE + 8, (cases.FAINT_PILE + 7) // 256)]
    if name == "dest":
        hid = c.hidden
        for q, t in c.targets[cases.AT].items():
            m = M[cases.AT + (q,)]
            for e in t.edges:
                where = {int(p): j for j, p in enumerate(m.pos)}
                gone = [j for j in (where[e - 1], where[e]) if hid[m.quad.splats[j]]]
                assert len(gone) == 1 and m.quad.dead(gone[0]) and gone[0] in m.quad.rejected, (q, e)
        reached = np.zeros((c.h, c.w), bool)
        for m in M.values():
            reached[m.quad.py, m.quad.px] |= (m.quad.a > 0).any(axis=0)
        assert reached.sum() < 32 * 32 and c.dest_rgba is not None
    if name == "shared":
        assert d.list_shift == 2 and len({rr.deep_ref.list_of(d, *b) for b in c.targets}) == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_pinned_share_and_the_models_own_centre(name, mode):
    """>= 95 % of the checked channel values pinned in every case, the model alone; the walk with every alpha at its centre - what a
    right kernel with exact alphas would leave - passes the comparison the GPU tests use."""
    c, d, M = models(name, mode)
    frame = np.zeros((c.h, c.w, 4), np.uint8) if c.dest_rgba is None else c.dest_rgba.copy()
    for m in M.values():
        frame[m.quad.py, m.quad.px] = rr.centre(m)[2].astype(np.uint8)
    bad, share, widest = rr.check_frame(frame, M, dest_rgba=c.dest_rgba, what=f"{name} {mode}")
    print(f"{name} {mode}: {len(M)} live quadrants, pinned share {share:.4f}, widest interval {widest}")
    assert bad == [], bad[:3]
    assert share >= PINNED and widest <= 1, (name, mode, share, widest)
    per_bin = min(np.mean([M[b + (q,)].pinned().mean() for q in range(4) if b + (q,) in M]) for b in c.targets)
    assert per_bin >= PINNED, (name, mode, per_bin)          # ... and in the targeted bins on their own


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_rop_emulating_oracle_lies_inside_the_full_walks_interval(name):
    c = cases.case(name)
    _, d, M = models(name, rr.FULL, pad=rr.PAD_UNFUSED)
    s = helpers.oracle_inputs(c.scene)
    ocam = oracle.make_camera(c.cam.model_view(), c.cam.projection, c.cam.position, c.w, c.h, 0, 0)
    (fb, _), = oracle.render_windows(ocam, *s, c.order, windows=[(0, 0, c.w, c.h)], rop8=True, depth=c.dest_depth, dst_rgba=c.dest_rgba)[0]
    frame = np.floor(np.clip(fb, 0, 1) * 255.0 + 0.5).astype(np.uint8)
    bad, share, widest = rr.check_frame(frame, M, dest_rgba=c.dest_rgba, what=f"{name} oracle")
    print(f"{name}: the oracle's frame inside the interval, pinned share {share:.4f}, widest {widest}")
    assert bad == [], bad[:3]
    assert share >= PINNED and widest <= 1, (name, share, widest)      # ... at the model's real sharpness


def test_every_mutation_is_caught_by_a_case_that_names_it():
    seen, listed = {}, set()
    for name, wants in cases.CATCHES.items():
        c = cases.case(name)
        for mode in sorted(set(wants.values())):
            _, d, M = models(name, mode)
            want = rr.predictions(M)
            for b, per in c.targets.items():
                Mbin = {q: M[b + (q,)] for q in range(4) if b + (q,) in M}
                edges = {q: t.edges for q, t in per.items()}
                for mut in rr.mutations(Mbin, edges):
                    listed.add(mut.name)
                    if wants.get(mut.name) != mode:
                        continue
                    pixel, integer = rr.caught(mut, Mbin, want[b])
                    counters_only = mut.name.startswith(cases.ONLY_COUNTERS)
                    ok = (pixel or counters_only) and (integer or not mut.changes_walk)
                    if counters_only:                        # only the counters can show it: EVERY instance of it must break one
                        assert integer, (name, mode, b, mut.q, mut.name)
                    if ok and (pixel or integer):
                        seen.setdefault(mut.name, set()).add(f"{name}/{mode}" + ("" if pixel else " (counters)"))
                    else:
                        seen.setdefault(mut.name, set())
                        print(f"NOT caught: {name} {mode} bin {b}: {mut.name} (pixel {pixel}, integer {integer}, changes the walk "
                              f"{mut.changes_walk})")
    for k in sorted(seen):
        print(f"{k}: {sorted(seen[k])}")
    named = {m for w in cases.CATCHES.values() for m in w}
    assert named <= set(seen), named - set(seen)
    assert listed <= named, f"mutations no case names: {listed - named}"
    assert all(seen[k] for k in named), [k for k in named if not seen[k]]


def test_interval_tightness_on_random_lists():
    """The simulation behind the model's claim to be sharp: lists of 64 .. 3000 survivors over 256 pixels, alphas uniform or with a
    Gaussian falloff up to 0.99 / 0.3 / 0.05, random colours.  Never wider than 1 step, the centre walk always inside, and the COLOUR
    channels pinned on >= 97 % of the values in all six classes at every depth.  The ALPHA channel (source 1) is asserted apart: it
    is pinned on >= 97 % wherever some fragments are loud, and under the faint lists while they are short.  alpha' = q8(a + (1 - a)
    alpha) only ever rises and STALLS once a (255 - alpha) < 0.5 (csrc/tile_blend.hip says so of the bounded mode's alpha): with
    alphas below 0.05 that is from 255 - alpha < 10 .. 20 on, reached after about ln(20 / 255) / ln(1 - 0.025) = 100 survivors; lo
    and hi then stall on the same byte or on neighbours, and nothing ever merges two stalled neighbours.  The open share of alpha
    therefore GROWS with the depth of a faint list (it is printed); what holds, and is asserted, is that it is never more than one
    step wide.  (The designed cases, alpha included, are held to 95 %.)"""
    rng = np.random.default_rng(11)
    worst_colour, worst_alpha, widest = {}, {}, 0
    for falloff in (False, True):
        for peak in (0.99, 0.3, 0.05):
            for S in (64, 300, 1000, 3000):
                colour, alpha, wide, inside = rr.simulate(rng, S, peak, falloff, pixels=256)
                print(f"S = {S:4d} peak {peak:.2f} {'falloff' if falloff else 'uniform'}: colour pinned {colour:.4f}, alpha pinned {alpha:.4f}, widest {wide}")
                assert inside and wide <= 1
                assert colour >= 0.97, (S, peak, falloff, colour)
                if peak >= 0.3 or S <= 64:
                    assert alpha >= 0.97, (S, peak, falloff, alpha)
                worst_colour[peak] = min(worst_colour.get(peak, 1.0), colour)
                worst_alpha[peak] = min(worst_alpha.get(peak, 1.0), alpha)
                widest = max(widest, wide)
    print(f"random lists: colour pinned >= {worst_colour}, alpha pinned >= {worst_alpha}, widest interval {widest}")
