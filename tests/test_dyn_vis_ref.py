"""CPU tier of the dynamic-mode visibility-culled sort (dyn_vis_cases.py): (a) a numpy restatement of the dynamic key, fed through
the host model of the three front ends (vis_front_ref.front_end), returns the sort oracle's list restricted to the raster oracle's
visible set, its count and its min / max for every case of the list at CPU-sized shapes; (b) every mutation of that model changes
the result of at least one case; and the conditions the scene construction promises, asserted with the oracles alone.

T = 16 workgroups here, so the sizes where the streaming front end takes a second and a third turn (T*2048+1 = 32769 and T*4096+1 =
65537 splats) stay below 70 k; the GPU tier takes T from the device."""
import numpy as np
import pytest

import dyn_vis_cases as dyn
import vis_front_cases as cases
import vis_front_ref as ref

T = 16
SIZES = cases.sizes(T)
SMALL_LABELS = ("1", "3", "33", "65", "4097")
BIG_LABELS = ("T*2048+1", "T*4096+1")
MUTATIONS = dyn.KEY_MUTATIONS + ("minmax_over_survivors",)
_SCENES = {}


def scene_of(n, layout, mode, odd_w=False):
    """The scene with the oracles' verdicts: drawn (raster oracle, every splat unhidden) and the sort oracle's list, keys, min / max."""
    key = (n, layout, mode, odd_w)
    if key not in _SCENES:
        if len(_SCENES) > 6:
            _SCENES.clear()
        s = dyn.make_scene(n, T, layout, mode, odd_w)
        s.drawn = dyn.oracle_visible(s, np.ones(n, dtype=bool))
        s.sorted = {n: dyn.oracle_sort(s, n)}
        _SCENES[key] = s
    return _SCENES[key]


def case_list():
    """(label, layout, mode, odd_w, pattern, R) as the GPU tier runs them, at the sizes this tier can afford."""
    for label in SMALL_LABELS:
        n = SIZES[label]
        for layout in dyn.LAYOUTS:
            for mode in dyn.MODES:
                for name in cases.pattern_names(n, T):
                    yield label, layout, mode, False, name, n
    for label in BIG_LABELS:
        for layout, mode in zip(dyn.LAYOUTS, dyn.MODES):
            for name in dyn.BIG_PATTERNS:
                yield label, layout, mode, False, name, SIZES[label]
    for label in ("4097", "T*2048+1"):
        n = SIZES[label]
        for mode in dyn.MODES:
            yield label, "runs", mode, False, "rand30", n - cases.SHORT[0]          # the short list
            for name in ("all", "rand30"):
                yield label, "random", mode, True, name, n                           # the sorter-only w variant


def model(s, want, R, front, mutation=None):
    """One sort through the host model of `front` with the numpy key: {list, kept, key_min, key_max, keep_bits}."""
    key_mut = mutation if mutation in dyn.KEY_MUTATIONS else None
    keys = dyn.model_keys(s, R, key_mut, survivors=want)
    front_mut = mutation if mutation in ref.MUTATIONS else None
    return ref.run_sequence(front, [(want, R)], s.count, keys, T, mutation=front_mut, precision=s.precision)[0]


def oracle_result(s, want, R):
    if R not in s.sorted:
        s.sorted[R] = dyn.oracle_sort(s, R)
    order, _, lohi = s.sorted[R]
    return {"list": order[want[order]], "kept": int(want[:R].sum()), "key_min": lohi[0], "key_max": lohi[1], "keep_bits": want[:R]}


def test_the_scene_keeps_its_promises():
    """With the oracles alone: the scene that draws nothing owns the key minimum and scene 1 the maximum; 0 < kept < n for every
    pattern that keeps anything at all (`none`, and `odd_turns` where no chunk has a second turn, keep nothing) from 33 splats up;
    on a keep-order mesh (storage = original order) the `runs` layout has 256-splat blocks without a survivor and blocks with some
    but not all; the boundaries of the `runs` layout sit where the docstring of dyn_vis_cases says; odd_w changes a tenth of the w."""
    for label in ("33", "65", "4097") + BIG_LABELS:
        n = SIZES[label]
        for layout in dyn.LAYOUTS:
            s = scene_of(n, layout, "int")
            _, keys, lohi = s.sorted[n]
            assert not s.drawn[s.real == dyn.K - 1].any() and (s.real == dyn.K - 1).any()
            assert s.drawn[list(dyn.protected_positions(n, T))].all()
            if n >= 4097:
                assert s.real[np.argmin(keys)] == dyn.K - 1 and s.real[np.argmax(keys)] == 1 and (keys.min(), keys.max()) == tuple(lohi)
            for name in cases.pattern_names(n, T) if n <= 4097 else dyn.BIG_PATTERNS:
                P = cases.pattern(name, n, T)
                want = dyn.oracle_visible(s, P)
                assert np.array_equal(want, P & s.drawn), (label, layout, name)           # per splat: one oracle call per rig suffices
                assert not P.any() or 0 < want.sum() < n, (label, layout, name)
            if layout == "runs" and n >= 4097:
                want = cases.pattern("rand30", n, T) & s.drawn
                per = np.add.reduceat(want.astype(np.int64), np.arange(0, n, 256))
                size = np.add.reduceat(np.ones(n, dtype=np.int64), np.arange(0, n, 256))
                assert (per == 0).any() and ((per > 0) & (per < size)).any()
    n = SIZES["T*2048+1"]
    b = dyn.run_boundaries(n, T)
    g = ref.geometry(n, T, "stream")
    assert any(v % 4 in (1, 2, 3) for v in b) and any(v % 4 == 0 and v % 256 for v in b)
    assert set(b) & set(g["turn_edges"]) and set(b) & set(g["chunk_edges"])
    assert set(b) <= set((np.nonzero(np.diff(dyn.scene_of(n, T, "runs").astype(np.int64)))[0] + 1).tolist())
    s = dyn.make_scene(4097, T, "random", "int", odd_w=True)
    assert 0.09 < (s.centres4[:, 3] != 1000).mean() <= 0.11
    s = dyn.make_scene(4097, T, "random", "float", odd_w=True)
    assert 0.09 < (s.centres4[:, 3] != 1.0).mean() <= 0.11


@pytest.mark.parametrize("label", SMALL_LABELS + BIG_LABELS)
def test_the_model_is_the_oracle(label):
    """(a) For every case of the list at this size: the numpy key equals the oracle's key position by position, and the model of
    every front end returns the oracle's restricted list, kept count, min / max and keep bits."""
    done = 0
    for lab, layout, mode, odd_w, name, R in case_list():
        if lab != label:
            continue
        s = scene_of(SIZES[label], layout, mode, odd_w)
        P = cases.pattern(name, s.count, T)
        want = dyn.oracle_visible(s, P)
        exp = oracle_result(s, want, R)
        assert np.array_equal(dyn.model_keys(s, R), s.sorted[R][1]), (layout, mode, odd_w, name, R)
        for front in ref.FRONTS:
            assert ref.same(model(s, want, R, front), exp), (layout, mode, odd_w, name, R, front)
        done += 1
    assert done


def test_every_mutation_is_detected_by_the_case_list():
    """(b) The mutation table (pytest -s prints it): per mutation, the cases whose result it changes.  static_key: the transforms
    ignored; scene0_row: scene 0's row for every splat; w_dropped: no w term; w_constant: 1000 / 1.0 instead of the w plane (only
    the odd_w cases can see it); scene_at_slot: the scene index read at the output slot instead of at the position;
    minmax_over_survivors: min / max over the survivors only (scene 3 draws nothing and owns the minimum).  A size above 4097 is
    tried only for a mutation no smaller case has caught."""
    table = {m: [] for m in MUTATIONS}
    tried = 0
    for label, layout, mode, odd_w, name, R in case_list():
        small = SIZES[label] <= 4097
        todo = [m for m in MUTATIONS if small or not table[m]]
        if not todo:
            continue
        s = scene_of(SIZES[label], layout, mode, odd_w)
        want = cases.pattern(name, s.count, T) & s.drawn
        exp = oracle_result(s, want, R)
        tried += 1
        for m in todo:
            if not ref.same(model(s, want, R, "stream", m), exp):
                table[m].append(f"{label}/{layout}/{mode}{'/odd_w' if odd_w else ''}/{name}/R={R}")
    print(f"\nmutation table ({tried} cases through the streaming front end's model):")
    for m, hits in table.items():
        print(f"  {m:24s} detected by {len(hits):4d} cases, first {hits[:3]}")
    assert all(table.values()), [m for m, hits in table.items() if not hits]
    assert all("odd_w" in h for h in table["w_constant"])
