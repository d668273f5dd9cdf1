"""CPU tier of the visibility-culled sort's front-end checks: the scene construction of vis_front_cases.py against the raster
oracle, the host model (vis_front_ref.py) against the sort oracle, and proof that the case list of the GPU tier bites - every
mutation of the model changes its output for at least one (size, pattern, path) of that list.  T = 512 workgroups here (an
MI355X's 2 x 256 CUs); the GPU tier takes T from the device."""
import numpy as np
import pytest

import oracle
import vis_front_cases as cases
import vis_front_ref as ref
from gaussiansplats3d_amd import util

T = 512
SIZES = cases.sizes(T)
_SCENES = {}


def scene_of(n):
    if n not in _SCENES:
        if len(_SCENES) > 2:
            _SCENES.clear()
        s = cases.make_scene(n, T)
        s.ci = util.integer_centers(s.centers)
        s.order, s.keys, _, s.lohi, _ = oracle.sort_indexes(np.arange(n, dtype=np.uint32), s.ci, s.cam.sort_mvp(), return_intermediates=True)
        _SCENES[n] = s
    return _SCENES[n]


def test_chunk_grid_and_geometry():
    """The cut the sizes are chosen for: one turn per workgroup up to T * 2048 positions, two (and empty workgroups) from T * 2048
    + 1, three from T * 4096 + 1; k_minmax_count's second span at T * 1024 + 1; k_mask_compact's second iteration and the derive
    pieces' second round at 2T * 4096 + 1."""
    assert ref.TURN == 2048 and ref.chunk_grid(1, ref.TURN, T) == (1, 2048)
    assert ref.chunk_grid(T * 2048, ref.TURN, T) == (T, 2048)
    g = ref.geometry(T * 2048 + 1, T, "stream")
    assert (g["len"], g["empty_chunks"], g["last_chunk"]) == (4096, T // 2 - 1, (T * 2048, T * 2048 + 1)) and not g["third_turn_edges"]
    assert ref.geometry(T * 4096 + 1, T, "stream")["third_turn_edges"] and not ref.geometry(T * 4096, T, "stream")["third_turn_edges"]
    assert ref.chunk_grid(T * 1024, ref.SPAN, T)[1] == 1024 and ref.chunk_grid(T * 1024 + 1, ref.SPAN, T)[1] == 2048
    assert ref.chunk_grid(2 * T * 4096, ref.SPAN, T)[1] == ref.COMPACT_ITER and ref.geometry(2 * T * 4096 + 1, T, "compact")["turn_edges"]
    assert ref.chunk_grid(2 * T * 4096 + 1, ref.UNIT["lazy"], T)[1] // ref.DERIVE_SUBS > ref.DERIVE_ROUND
    assert (cases.NONCOARSE + 255) // 256 == ref.COARSE_BLOCKS + 1
    for n in (4097, T * 2048 + 1, 2 * T * 4096 + 1):               # the single-survivor positions are distinct and in front
        e = cases._edge_positions(n, T)
        assert len(e) >= 4 and not cases.behind_set(n, T)[list(e.values())].any()


@pytest.mark.parametrize("label", [k for k, v in SIZES.items() if v <= 4097])
def test_constructed_mask_is_the_oracles_and_the_model_is_the_oracle_list(label):
    """For every pattern of a small size: oracle.project's `visible` is exactly P & ~behind (and the complement under visible =
    [0, 1]); the unmutated model of every front end returns the sort oracle's list restricted to it, its min / max over all
    positions, the count and the keep bits - also for the short lists."""
    n = SIZES[label]
    s = scene_of(n)
    for name in cases.pattern_names(n, T):
        P = cases.pattern(name, n, T)
        want = P & ~s.behind
        assert np.array_equal(cases.oracle_visible(s, P), want), name
        assert np.array_equal(cases.oracle_visible(s, P, (0, 1)), ~P & ~s.behind), name
        for R in [n] + [n - d for d in cases.SHORT if n > 4000]:
            order, keys, _, lohi, _ = oracle.sort_indexes(np.arange(R, dtype=np.uint32), s.ci, s.cam.sort_mvp(), return_intermediates=True)
            for front in ref.FRONTS:
                got = ref.run_sequence(front, [(want, R)], n, keys, T)[0]
                assert np.array_equal(got["list"], order[want[order]]), (name, R, front)
                assert (got["kept"], got["key_min"], got["key_max"]) == (int(want[:R].sum()), *lohi), (name, R, front)
                assert np.array_equal(got["keep_bits"], want[:R])


def test_constructed_mask_and_model_at_three_turns():
    """The same at 2T * 4096 + 1 splats for two patterns; the minimum over the survivors is not the minimum over all positions
    (the splats behind the camera have the smallest keys), so a front end that reduces over survivors only is caught."""
    n = SIZES["2T*4096+1"]
    s = scene_of(n)
    for name in ("rand30", "stream:odd_turns"):
        P = cases.pattern(name, n, T)
        want = P & ~s.behind
        assert np.array_equal(cases.oracle_visible(s, P), want), name
        assert int(s.keys[want].min()) > s.lohi[0] and len(np.unique(ref.buckets(s.keys[want], *s.lohi))) < want.sum() // 8
        for front in ref.FRONTS:
            got = ref.run_sequence(front, [(want, n)], n, s.keys, T)[0]
            assert np.array_equal(got["list"], s.order[want[s.order]]) and got["kept"] == int(want.sum())
            assert (got["key_min"], got["key_max"]) == tuple(s.lohi)


def gpu_case_list():
    """(size label, n, pattern, R) as the GPU tier runs them: every pattern at every size (R = n), the short lists at PATH_SIZES -
    each as the lifecycle sequence A, complement of A, A."""
    for label, n in SIZES.items():
        for name in cases.pattern_names(n, T):
            yield label, n, name, n
            if label in cases.PATH_SIZES and name in ("all", "rand30", "mod5", "last") and n > 4000:
                for d in cases.SHORT:
                    yield label, n, name, n - d


def test_every_mutation_is_detected_by_the_case_list():
    """The mutation table: per mutation of the model, the cases of the GPU list whose result it changes (a case = the sequence
    pattern, complement, pattern through one front end).  Every mutation must be detected; the table is printed (pytest -s).
    Sizes above 4097 are tried only for a mutation no smaller case has caught, with the random 30 % pattern, and only until one
    catches it: the counts say how many of the cases TRIED detect a mutation, not how many of the list would (turn_parity_reused
    needs a chunk of three turns with survivors behind the third, which the lists up to 4097 positions do not have).  That mutation
    is a deterministic stand-in for a single-buffered s_turn - turn t reads what turn t - 2 left - not the race itself."""
    table = {m: [] for m in ref.MUTATIONS}
    tried = 0
    for label, n, name, R in gpu_case_list():
        small = n <= 4097
        todo = [m for m in ref.MUTATIONS if small or not table[m]]
        if not todo or not (small or name == "rand30"):
            continue
        s = scene_of(n)
        keys = s.keys if R == n else oracle.sort_indexes(np.arange(R, dtype=np.uint32), s.ci, s.cam.sort_mvp(), return_intermediates=True)[1]
        P = cases.pattern(name, n, T)
        a, b = P & ~s.behind, ~P & ~s.behind
        steps = [(a, R), (b, R), (a, R)]
        for front in ref.FRONTS:
            base = ref.run_sequence(front, steps, n, keys, T)
            tried += 1
            for m in todo:
                mut = ref.run_sequence(front, steps, n, keys, T, mutation=m)
                if not all(ref.same(x, y) for x, y in zip(base, mut)):
                    table[m].append(f"{label}/{name}/R={R}/{front}")
    print(f"\nmutation table ({tried} (size, pattern, list length, front end) sequences of the GPU case list):")
    for m, hits in table.items():
        print(f"  {m:26s} detected by {len(hits):4d} cases, first {hits[:3]}")
    assert all(table.values()), [m for m, hits in table.items() if not hits]
