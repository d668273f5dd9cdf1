"""No GPU: the host model of the chunked composite (tests/deep_ref.py) and the designed scenes (tests/deep_cases.py), from records
of the CPU oracle's vertex stage and the binner's host model.  Everything the GPU tests (tests/test_gpu_deep_edges.py) rely on is
asserted here: the chunk table, that every case reaches its survivor counts and list lengths exactly, that no (splat, quadrant)
pair lies in quadrant_ref's band, that ambiguous pixels are rare and never under a marker, which quadrants saturate - and that each
mutation of interest at every targeted chunk edge moves a checked pixel by >= 8/255 AND is rejected by the very comparison
function the GPU tests use (deep_ref.compare_values), the mutated model's pixels standing in for a frame.

Printed (pytest -s): the largest per-pixel tolerance any tested pixel receives and the smallest movement over all
(case, edge, mutation) triples, both in 1/255 - the figures DESIGN.md's parity section records - when the module is done."""
import numpy as np
import pytest

import deep_cases as cases
import deep_ref as dr

MOVE = 8.0                                      # 1/255: what every mutation must move some checked pixel by
TOL_32 = 0.5 + 255.0 * dr.DELTA + 255.0 * dr.T_EPS * (dr.CHUNKS_MAX + 1)      # the tolerance of a 32-chunk quadrant without ambiguity: 1.36


@pytest.fixture(scope="module", autouse=True)
def figures():
    """The two figures, over whatever part of the module ran; printed when the module is done."""
    f = {"tolerance": 0.0, "movement": np.inf, "triples": 0, "void": 0}
    yield f
    print(f"\nlargest per-pixel tolerance {f['tolerance']:.3f} / 255, smallest movement {f['movement']:.1f} / 255 over "
          f"{f['triples']} (case, edge, mutation) triples ({f['void']} more touch only survivors the depth plane hides)")


def model_of(name, **kw):
    """(case, draw, quadrants): one case at a time - a quadrant holds [S, 256] float64 planes."""
    c = cases.case(name)
    d = cases.cpu_draw(c, **kw)
    return c, d, cases.quads_of(d)


def test_chunk_table_brute_force_against_the_headers_closed_forms():
    """gs_internal.hpp's static_assert, value by value, and the closed forms of gs_chunk_size / _first / _count restated here
    ONLY to be compared with the brute force over the table."""
    assert dr.BOUNDARIES[:10] == [1024, 1280, 1536, 1792, 2048, 2560, 3072, 3584, 4096, 5120]
    assert len(dr.BOUNDARIES) == dr.CHUNKS_MAX - 1 and dr.BOUNDARIES[-1] == 26624
    assert dr.chunk_first(5) == 2048 and dr.chunk_first(9) == 4096
    assert [dr.chunk_count(s) for s in (1025, 2048, 2049, 4096, 4097, 1 << 20)] == [2, 5, 6, 9, 10, dr.CHUNKS_MAX]
    size = lambda c: 1024 if c == 0 else 256 if c < 5 else 512 if c < 9 else 1024
    first = lambda c: 0 if c == 0 else 1024 + (c - 1) * 256 if c < 5 else 2048 + (c - 5) * 512 if c < 9 else 4096 + (c - 9) * 1024
    count = lambda s: (0 if s == 0 else 1 if s <= 1024 else 1 + (s - 1024 + 255) // 256 if s <= 2048 else 5 + (s - 2048 + 511) // 512
                       if s <= 4096 else min(9 + (s - 4096 + 1023) // 1024, dr.CHUNKS_MAX))
    for c in range(dr.CHUNKS_MAX):
        assert dr.chunk_first(c) == first(c)
        if c < dr.CHUNKS_MAX - 1:
            assert dr.SIZES[c] == size(c) and dr.chunk_of(first(c)) == c and dr.chunk_of(first(c) + size(c) - 1) == c
    for s in list(range(0, 6200)) + [b + d for b in dr.BOUNDARIES for d in (-1, 0, 1)] + [30000, 65536, 65537, 1 << 20]:
        assert dr.chunk_count(s) == count(s), s
    assert dr.chunk_of(26623) == 30 and dr.chunk_of(26624) == 31 and dr.chunk_of(10 ** 7) == 31


def test_frames_have_at_least_40_blend_bins():
    for name in cases.NAMES:
        c = cases.case(name)
        assert ((c.w + 31) // 32) * ((c.h + 31) // 32) >= 40
        assert c.list_shift == 1
        assert c.scene.count == c.order.shape[0]
    c = cases.case("ladder_a")                               # the array builder IS quadrant_cases.splat
    for k in (0, 1023, 4000):
        one = cases.quadrant_cases.splat(c.cam, *c.items[k][:4], depth=cases.D0 + cases.STEP * c.depth_index[k])
        assert np.array_equal(one[0], c.scene.centers[k]) and np.allclose(one[1], c.scene.cov[k], rtol=3e-7, atol=0)


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_conditions(figures, name):
    """Target counts, list lengths, the quadrant band, ambiguous pixels, saturation and the edges of the issue's list, each
    reached by an assertion on the model's own counts."""
    c, d, Q = model_of(name)
    conditions(name, c, d, Q, figures)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_mutation_moves_a_checked_pixel_and_fails_the_gpu_tests_comparison(figures, name):
    c, d, Q = model_of(name)
    mutations(name, c, Q, figures)


def test_figures(figures):
    """The two figures DESIGN.md records, over the cases above (selected alone: over ladder_a): every mutation moves a pixel by
    more than ten times the largest tolerance."""
    if not figures["triples"]:
        c, d, Q = model_of("ladder_a")
        conditions("ladder_a", c, d, Q, figures)
        mutations("ladder_a", c, Q, figures)
    assert figures["triples"] > 0 and figures["movement"] >= 10.0 * max(TOL_32, figures["tolerance"]), figures


def conditions(name, c, d, Q, figures):
    seen_tol = 0.0
    for (bx, by), want in c.list_len.items():
        assert dr.list_of(d, bx, by)[1] == want, (name, bx, by)
    for (bx, by), per in c.targets.items():
        for q, t in per.items():
            m = Q[(bx, by, q)]
            assert m.S == t.S, (name, bx, by, q, m.S, t.S)
            assert m.non_saturating() == (not t.saturating), (name, bx, by, q)
            marks = cases.marker_pixels(c, m)
            assert not (m.amb.any(axis=0) & marks).any(), (name, bx, by, q)
            if t.edges:
                assert marks.sum() == 20
            if not t.saturating:                             # T after every chunk edge: no chunk's stop rule can have fired
                assert all(T.max() >= dr.NON_SATURATING_T for T in m.T_after_edges().values()), (name, bx, by, q)
    for key, m in Q.items():                                 # every live quadrant with a list, named by the case or not
        assert m.in_band == 0, (name, key, m.in_band)
        assert m.amb.any(axis=0).mean() <= 0.02 if m.px.size else True, (name, key)
        named = c.targets.get(key[:2], {}).get(key[2])
        assert m.non_saturating() == (not (named is not None and named.saturating)), (name, key)
        seen_tol = max(seen_tol, float(m.tolerance().max(initial=0.0)))
        if named is None:
            m.release()
    figures["tolerance"] = max(figures["tolerance"], seen_tol)
    print(f"{name}: {c.scene.count} splats, {len(Q)} live quadrants with a list, largest tolerance {seen_tol:.3f} / 255")
    # the edges this case is there for
    S = {k: m.S for k, m in Q.items()}
    if name == "ladder_a":
        assert sorted(S.values()) == [1023, 1024, 1025, 1281]
    if name == "ladder_b":
        assert sorted(S.values()) == [2048, 2049, 4096, 4097]
    if name == "ladder_c":
        assert sorted(S.values()) == [0, 1, 5120, 5121] and Q[(3, 2, 3)].S == 0 and dr.live(d, 3, 2, 3)
        assert Q[(3, 2, 3)].chunks == 0 and not dr.rgba_of(*Q[(3, 2, 3)].value()).any()
    if name == "tail":
        assert sorted(S.values()) == [0, 26624, 26625, 30000] and dr.list_of(d, 4, 1)[1] <= dr.LIST_CAP
        assert [dr.chunk_count(s) for s in (26624, 26625, 30000)] == [31, 32, 32]
        assert dr.chunk_of(26624) == 31 and dr.chunk_of(29999) == 31          # chunk 31 holds 1 and 3376 survivors: unbounded
        t27 = Q[(4, 1, 1)].T_at(27000)                         # pixels the fills DO cover still hold T >= 1e-2 after 27 000 of them
        assert ((t27 >= dr.NON_SATURATING_T) & (t27 < 0.9)).sum() >= 8 and (t27 < 1e-6).sum() >= 8      # (and their middle is long gone)
    if name == "cap":
        assert dr.list_of(d, 1, 1)[1] == dr.LIST_CAP and dr.list_of(d, 6, 3)[1] == dr.LIST_CAP + 1
        assert dr.LIST_CAP // dr.RLEN == 64
    if name == "sparse":
        m = Q[(2, 3, 0)]
        begin, n = dr.list_of(d, 2, 3)
        assert n == 60000 and m.S == 1500
        pos = np.nonzero(np.isin(d.splat_of_slot()[d.entries[begin:begin + n]], m.splats))[0]
        assert pos.shape[0] == 1500
        p = int(pos[1024])                                   # the chunk's first survivor: mid-window, mid-range, survivors before
        assert p % 64 == 32 and (p % dr.RLEN) == 512 + 32 and p // dr.RLEN == 40
        in_range = pos[(pos >= 40 * dr.RLEN) & (pos < p)]
        assert in_range.shape[0] >= 20 and (in_range >= p - 32).sum() >= 20     # skip > 0, counted down inside the window itself
        two_windows = np.array([((pos >= w * 64) & (pos < (w + 2) * 64)).sum() for w in range(n // 64)])
        assert (two_windows > 64).sum() >= 5                                    # the queue carries more than 64 pending survivors
    if name == "edge":
        assert c.w % 32 == 16 and c.h % 32 == 16
        assert [dr.live(d, 8, 5, q) for q in range(4)] == [True, False, False, False]
        assert [dr.live(d, 8, 2, q) for q in range(4)] == [True, False, True, False]
        for rows, want in (((0, 5), [True, False, False, False]), ((5, 11), [False, False, True, False])):
            assert [dr.live(d, 8, 2, q, rows) for q in range(4)] == want      # the strips' cut passes through bin (8, 2)
        assert all(dr.list_of(d, *b)[1] >= 4 * 1024 for b in c.targets)
    if name == "saturating":
        m = Q[(3, 2, 0)]
        k = m.saturation_point(dr.T_EPS / 4)
        assert k is not None and dr.chunk_of(k - 1) == 2 and m.S - k >= 3000   # saturates inside chunk 2, 3000 more behind
        local = np.cumprod(1.0 - m.a[1280:1536], axis=0).max(axis=1)           # chunk 2 from T = 1: it saturates ON ITS OWN
        assert (local <= dr.T_EPS / 4).any()
    if name == "depth":
        hid = c.hidden
        _, d0, Q0 = model_of(name, with_dest=False)
        for (bx, by), per in c.targets.items():
            for q, t in per.items():
                m, m0 = Q[(bx, by, q)], Q0[(bx, by, q)]
                assert m0.S == m.S                                             # hidden survivors still count towards the edges
                assert 0.3 < hid[m.splats].mean() < 0.36                       # every third survivor lies behind the plane ...
                plane = (m.px % 16) >= 8
                assert not m.a[hid[m.splats]][:, plane].any() and m.a[hid[m.splats]][:, ~plane].any()   # ... and shows only left of it
                marks = cases.marker_pixels(c, m)
                want, bare = dr.rgba_of(*m.value()), dr.rgba_of(*m0.value())
                assert np.abs(want - bare)[marks].max() >= MOVE                # the plane shows AT the marker pixels
                for b in t.edges:
                    pair = [k for k in (b - 1, b) if k < m.S]
                    gone = [k for k in pair if hid[m.splats[k]]]
                    assert len(gone) == 1 and not hid[m.splats[[b - 4, b - 3]]].any()
                    k = gone[0]                                                # the hidden marker of the edge: rejected at EVERY pixel it covers,
                    assert m.dead(k) and not m0.dead(k) and k in m.rejected    # several of them marker pixels where it would be loud
                    assert ((m.rejected[k] > 0.3) & marks & plane & (m.a[k] == 0.0) & (m0.a[k] > 0.3)).sum() >= 4
                    seen = [j for j in pair if j != k]
                    assert all(not m.dead(j) and (m.a[j][plane] > 0.3).any() for j in seen)    # its partner passes under the same plane
                m0.release()


def mutations(name, c, Q, figures):
    smallest = np.inf
    for (bx, by), per in c.targets.items():
        for q, t in per.items():
            m = Q[(bx, by, q)]
            want = dr.rgba_of(*m.value())
            assert dr.compare_values(np.floor(want + 0.5), m)[0] == []         # the model itself, rounded as a frame is, passes
            for b in t.edges:
                live = 0
                for what, (C, T), touched in m.mutations(b):
                    got = dr.rgba_of(C, T)
                    move = float(np.abs(got - want).max())
                    if any(m.dead(k) for k in touched):        # a survivor the plane hides everywhere: nothing a frame could show
                        assert name == "depth" and move < MOVE
                        figures["void"] += 1
                        continue
                    live += 1
                    figures["triples"] += 1
                    smallest = min(smallest, move)
                    assert move >= MOVE, (name, bx, by, q, b, what, move)
                    bad, worst, _ = dr.compare_values(np.floor(got + 0.5), m, what=what)
                    assert bad and worst > 4.0, (name, bx, by, q, b, what, worst)
                assert live >= 1, (name, bx, by, q, b)
                if name == "depth":                            # the hidden marker of every edge, composited as if it passed, is loud
                    assert any(what.startswith("re-admit") for what, _, _ in m.mutations(b)), (name, bx, by, q, b)
            m.release()
    figures["movement"] = min(figures["movement"], smallest)
    tol = max(TOL_32, figures["tolerance"])
    print(f"{name}: smallest movement {smallest:.1f} / 255")
    assert smallest >= MOVE and smallest >= 10.0 * tol, (smallest, tol)      # more than ten times the largest tolerance
