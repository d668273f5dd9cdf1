"""The proof behind tests/test_gpu_sort_chains.py, on a machine without a GPU: the matrix of sort_chain_cases.py, together with the
children of tests/tools/sort_chain_child.py, reaches every radix pass chain csrc/sort_plan.cpp can plan for precisions 10..24 and
payloads of up to 25 bits - so a chain nobody runs on the device fails HERE, when plan_passes learns a new one - and every cell is
what it claims to be: its edge pairs straddle their edges, its lists hold the payload whose top bit stands alone, the oracle alone
sorts it, and float precision 24 comes both with and without a clamped bucket."""
import collections
import ctypes as C

import numpy as np
import pytest

import known_range_cases as kr
import oracle
import sort_chain_cases as cc
import sort_plan_cases as sc
import sort_plan_ref as ref

CELLS = cc.cells()
CHILDREN = {sw: cc.child_cells(sw) for sw in cc.SWITCHES}

# What the enumeration leaves out, by name: nothing else is excluded.
EXCLUSIONS = {
    "chunk_grid_0": "radix_chunk_grid_for(Rs) == 0 takes a list of more than 2048 * 3 * 4096 (25 M) keys",
    "val_bits_above_25": "a payload of more than 25 bits takes more than 2^25 uploaded splats (or a bound mesh that large)",
}
MAX_VAL_BITS = 25


def _library():
    """plan(inputs) through the library's pure-host entry gs_debug_sort_plan (loaded as tests/test_sort_plan.py loads it: a library
    that is missing or does not load is an error, not a skip)."""
    import gaussiansplats3d_amd as g
    fn = g.load().gs_debug_sort_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(sc.PlanIn), C.POINTER(sc.PlanOut)]

    def plan(inputs):
        s, out = sc.to_struct(inputs), sc.PlanOut()
        assert fn(C.byref(s), C.byref(out)) == 0
        return sc.out_from_struct(out)
    return plan


def _uploaded_for(val_bits):
    return 2 if val_bits == 1 else (1 << (val_bits - 1)) + 1  # last_splat = 2^(val_bits - 1): that bit alone


def enumerate_inputs():
    """Every (mode, precision, val_bits, list class, switch) a sorter can be asked for within the exclusions."""
    I, D = ref.SORT_INTEGER, ref.SORT_DYNAMIC
    classes = [dict(flags=I), dict(flags=I, sort="third"), dict(flags=I, list=ref.LIST_HOST), dict(flags=I, frustum_cull=1),
               dict(flags=I, frustum_cull=1, list=ref.LIST_HOST), dict(flags=I | D), dict(flags=I, precomputed=ref.PRE_HOST),
               dict(flags=0), dict(flags=0, list=ref.LIST_HOST), dict(flags=0, frustum_cull=1), dict(flags=0, precomputed=ref.PRE_HOST)]
    for cls in classes:
        for precision in (cc.INT_PRECISIONS if cls["flags"] & I else cc.FLOAT_PRECISIONS):
            for val_bits in range(1, MAX_VAL_BITS + 1):
                u = _uploaded_for(val_bits)
                n = min(u, cc.LIST_LEN) if cls.get("list") else u
                for sw in ({}, {"sw_no_pack": 1}, {"sw_no_chunk": 1}):
                    kw = {k: v for k, v in cls.items() if k != "sort"}
                    yield sc.make_inputs(precision=precision, uploaded=u, render_count=n, sort_count=max(n // 3, 1) if cls.get("sort") else n, **kw, **sw)


def test_the_exclusions_are_the_only_ones():
    seen = set()
    for i in enumerate_inputs():
        pl = ref.sort_plan(i)
        assert pl["Rs"] > 0
        assert pl["val_bits"] <= MAX_VAL_BITS, EXCLUSIONS["val_bits_above_25"]
        assert ref.radix_chunk_grid_for(pl["Rs"]) != 0, EXCLUSIONS["chunk_grid_0"]
        seen.add((i["precision"], pl["val_bits"]))
    assert seen == {(p, v) for p in cc.FLOAT_PRECISIONS for v in range(1, MAX_VAL_BITS + 1)}
    # what chunk_grid_0 leaves out changes no chain within 25 bits: the first such list is longer than 2^24 + 1, so its payload
    # has 25 bits, which rules chunk staging out by itself - the same chain on either side of that length
    first = 2048 * 3 * 4096 + 1
    assert ref.radix_chunk_grid_for(first - 1) != 0 and ref.radix_chunk_grid_for(first) == 0 and first > (1 << 24) + 1
    for precision in cc.FLOAT_PRECISIONS:
        a, b = (ref.sort_plan(sc.make_inputs(flags=0, precision=precision, n=n)) for n in (first - 1, first))
        assert a["val_bits"] == b["val_bits"] == 25 and cc.shape(a) == cc.shape(b) and not any(p["chunked"] for p in b["pass"])


def test_the_model_enumerates_what_the_library_plans():
    plan = _library()
    for i in enumerate_inputs():
        assert not sc.differences(plan(i), ref.sort_plan(i)), i
        assert cc.chain_key(i, plan) == cc.chain_key(i)


def possible_keys():
    keys = {}
    for i in enumerate_inputs():
        keys.setdefault(cc.chain_key(i), (i["precision"], i["uploaded"], i["flags"], i["list"], i["sw"]["no_pack"], i["sw"]["no_chunk"]))
    return keys


def unreached(cells, children):
    """Chains plan_sort can produce that neither the matrix (no switch) nor the child of the switch that makes them reaches."""
    main = cc.reached(cells)
    by_switch = {cc.SWITCHES[sw]: cc.reached(cl, sw) for sw, cl in children.items() if cc.SWITCHES[sw]}
    out = []
    for key, example in possible_keys().items():
        on = key[1]
        got = main if not on else by_switch[on[0]]
        if key not in got:
            out.append((key, example))
    return out


def test_the_matrix_reaches_every_pass_chain():
    keys = possible_keys()
    assert len({k[0] for k in keys}) >= 8                    # (two- and three-pass chains: packed, chunk-staged or not, KV16, KV32, never packed)
    assert unreached(CELLS, CHILDREN) == []


# -------------------------------------------------------------------------------------------------
# the rows the matrix was asked for, written down from the rule and not from sort_chain_cases
# -------------------------------------------------------------------------------------------------
def facts(cells):
    """Counter of (mode, precision, dynamic, data, dense, u, sort) over every sort of the cells."""
    out = collections.Counter()
    for c in cells:
        for u, sorts in c["steps"]:
            for s in sorts:
                out[(c["mode"], c["precision"], c["dynamic"], c["data"], c["dense"], u, s)] += 1
    return out


def required():
    F, P, M, E = cc.FULL, cc.PARTIAL, cc.PERM, cc.EDGE
    need = collections.Counter()
    for n in (4097, 24577):
        for data in ("gauss", "grid"):
            for p in range(10, 21):
                for s, k in (((F, 0, 0), 2), ((P, 0, 0), 1), ((M, 0, 0), 1), ((F, 1, 0), 1), ((M, 1, 0), 1)):
                    need[("int", p, False, data, True, n, s)] = k
            for p in range(10, 25):
                need[("float", p, False, data, True, n, (F, 0, 0))] = 1
        for p in (10, 13, 17, 20, 24):
            if p <= 20:
                need[("int", p, True, "gauss", True, n, (F, 0, 0))] = 1
                need[("int", p, False, "gauss", True, n, (F, 0, 1))] = 1
            need[("float", p, False, "gauss", True, n, (F, 0, 1))] = 1
    edges = [("int", 16, 1 << 24), ("int", 10, 1 << 24), ("float", 24, 1 << 24)]
    edges += [("int", p, 1 << (40 - p)) for p in (17, 18, 19, 20)] + [("float", p, 1 << (40 - p)) for p in (21, 22, 23, 24)]
    for mode, p, e in edges:
        for u in (e, e + 1):
            for s in ((E, 0, 0), (E, 1, 0), (E, 0, 1)):
                need[(mode, p, False, "gauss", False, u, s)] = 1
    for p in (16, 10):                                       # payload bit 23 alone through the chunk-staged last pass
        need[("int", p, False, "gauss", False, (1 << 23) + 1, (E, 0, 0))] = 1
    need[("int", 16, False, "gauss", False, (1 << 23) + 1, (F, 0, 0))] = 1   # the one large identity sort
    return need


def missing(cells, children):
    have = facts(cells)
    return [(f, k) for f, k in required().items() if have[f] < k] + unreached(cells, children)


def test_every_row_asked_for_is_there_and_none_can_go():
    assert missing(CELLS, CHILDREN) == []
    need = required()
    for k, cell in enumerate(CELLS):
        rest = CELLS[:k] + CELLS[k + 1:]
        have = facts(rest)
        assert any(have[f] < n for f, n in need.items()) or unreached(rest, CHILDREN), f"{cell['name']} can be removed unnoticed"
    # a row of a cell, too: float 24 without 2^24 + 1 loses the chain that never packs, integer 16 without 2^24 the 24-bit payload
    # under a packed, chunk-staged pass 0
    for name, u in (("edge_float_p24", (1 << 24) + 1), ("edge_int_p16", 1 << 24)):
        cut = [dict(c, steps=tuple(s for s in c["steps"] if s[0] != u)) if c["name"] == name else c for c in CELLS]
        assert facts(cut) != facts(CELLS) and missing(cut, CHILDREN)
    # ... and for those two the pass-chain proof alone notices
    cut = [dict(c, steps=tuple(s for s in c["steps"] if s[0] != (1 << 24) + 1)) if c["name"] == "edge_float_p24" else c for c in CELLS]
    assert any(key[0][0] == 3 and all(p[1] != ref.OUT_PACKED for p in key[0][1:]) and not key[1] for key, _ in unreached(cut, CHILDREN))
    for sw in ("GSPLAT_NO_SORT_CHUNK", "GSPLAT_NO_SORT_PACK"):
        assert unreached(CELLS, dict(CHILDREN, **{sw: []})), f"the child of {sw} reaches chains nothing else does"


def test_cell_names_are_unique_and_sorters_fit_their_modes():
    names = [c["name"] for c in CELLS]
    assert len(names) == len(set(names))
    for c in CELLS + [c for cl in CHILDREN.values() for c in cl]:
        assert c["precision"] in (cc.INT_PRECISIONS if c["mode"] == "int" else cc.FLOAT_PRECISIONS)
        us = [u for u, _ in c["steps"]]
        assert us == sorted(set(us)) and c["max_count"] == us[-1]   # (set_uploaded_count only grows a sorter)
        for u, sorts in c["steps"]:
            for kind, cull, pre in sorts:
                assert not (cull and (pre or c["dynamic"] or kind == cc.PARTIAL)), "a per-splat cull needs a full sort of a static scene"
                assert 0 < cc.counts(u, kind)[1] <= cc.counts(u, kind)[0] <= u, "the sorter clamps a sort's counts to `uploaded`"
    large = [c for c in CELLS if c["max_count"] > (1 << 23) + 1]
    assert all(c["max_count"] == (1 << 24) + 1 for c in large) and len(large) <= 4


def test_every_edge_pair_straddles_its_edge():
    seen = 0
    for c in CELLS + [c for cl in CHILDREN.values() for c in cl]:
        if c["dense"] or c["kind"] == "big":
            continue
        us = [u for u, _ in c["steps"]]
        for e in cc.EDGES.get((c["mode"], c["precision"]), ()):
            if e not in us:
                continue                                       # (a child's row with its own steps)
            assert e + 1 in us, c["name"]
            a, b = (ref.sort_plan(cc.plan_inputs(c, u, (cc.EDGE, 0, 0))) for u in (e, e + 1))
            assert b["val_bits"] == a["val_bits"] + 1
            flips = a["pass"][0]["out"] != b["pass"][0]["out"] or [p["chunked"] for p in a["pass"]] != [p["chunked"] for p in b["pass"]]
            assert flips, f"{c['name']}: nothing changes between {e} and {e + 1}"
            seen += 1
    assert seen >= len(cc.EDGES)


@pytest.fixture(scope="module")
def oracle_runs():
    """Every sort of every cell - the matrix and the rows only a child runs - through the oracle alone, once:
    [(cell, u, sort, arguments, list, clamped, status, clamped among the positions a cull keeps | None)]."""
    out = []
    names = {c["name"] for c in CELLS}
    extra = {c["name"]: c for cl in CHILDREN.values() for c in cl if c["name"] not in names}
    assert len(extra) == 3                                   # (the other child rows ARE rows of the matrix: same name, same data)
    for c in CELLS + list(extra.values()):
        host = cc.Host(c)
        for u, sorts in c["steps"]:
            host.advance(u)
            for k, sort in enumerate(sorts):
                a = host.sort_args(u, sort, k)
                lst, keys, _, (lo, hi), st = host.oracle(a)
                s0 = a["render_count"] - a["sort_count"]
                kept = None
                if a["cull"]:
                    keep = oracle.frustum_keep(a["mvp"], host.centers, a["listed"], host.use_int)
                    kept = oracle.count_clamped(keys[keep], lo, hi, c["precision"])
                out.append((c, u, sort, a, lst, oracle.count_clamped(keys[s0:], lo, hi, c["precision"]), st, kept))
    return out


def test_the_oracle_alone_sorts_every_cell(oracle_runs):
    for c, u, sort, a, lst, clamped, st, _ in oracle_runs:
        what = (c["name"], u, sort)
        assert np.array_equal(np.sort(lst), np.sort(a["listed"][:a["render_count"]])), what
        assert st == (1 if clamped else 0), what
        if sort[0] == cc.EDGE:
            assert len(a["indexes"]) == cc.LIST_LEN and (a["indexes"] == u - 1).any() and a["indexes"].max() == u - 1, what
            assert (a["indexes"] < cc.SPAN).any()
        if a["precomputed"] is not None:
            assert len(a["precomputed"]) == u


def test_float_24_comes_with_and_without_a_clamped_bucket(oracle_runs):
    """At 24 bits fp32 rounding can put the farthest splat into bucket `range`: the sorter clamps and reports it.  The matrix holds
    sorts where that happens and sorts where it does not (the seeds are the cells' names: checked here, not hoped for)."""
    f24 = [r for r in oracle_runs if r[0]["mode"] == "float" and r[0]["precision"] == 24 and r[0] in CELLS]
    p24 = [(c["name"], u, sort, clamped) for c, u, sort, _, _, clamped, _, _ in f24 if not sort[1]]
    assert any(k > 0 for *_, k in p24) and any(k == 0 for *_, k in p24), p24
    # under the frustum cull the sorter counts the clamps of the positions it keeps: some culled sort keeps one, some keep none
    culled = [(c["name"], u, sort, kept) for c, u, sort, _, _, _, _, kept in f24 if sort[1]]
    assert any(k > 0 for *_, k in culled) and any(k == 0 for *_, k in culled), culled
    below = [r[5] for r in oracle_runs if r[0]["precision"] <= 20]
    assert below and not any(below)


def test_the_oracle_counts_clamps_as_the_integer_formula_does():
    rng = np.random.default_rng(11)
    for precision in (10, 16, 20, 23, 24):
        for k in range(20):
            keys = rng.integers(-(1 << 27), 1 << 27, size=500).astype(np.int32)
            lo, hi = int(keys.min()), int(keys.max())
            assert oracle.count_clamped(keys, lo, hi, precision) == kr.expected_clamps(keys, lo, hi, precision)
    keys = np.full(9, 5, dtype=np.int32)
    assert oracle.count_clamped(keys, 5, 5, 16) == 0          # hi == lo: NaN, bucket 0, nothing clamped
    # a range narrower than the keys (what a stale known range would do): both count what falls outside
    keys = np.arange(-50, 150, dtype=np.int32)
    assert oracle.count_clamped(keys, 0, 100, 10) == kr.expected_clamps(keys, 0, 100, 10) > 0
