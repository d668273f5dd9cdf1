"""The matrix of tests/test_sort_chains.py (the CPU proof that it reaches every pass chain), tests/test_gpu_sort_chains.py (which runs
it) and tests/tools/sort_chain_child.py (which runs its edge rows under a switch): every radix pass chain csrc/sort_plan.cpp can
plan, run on the device at the payload widths and precisions where a shift or a mask can be wrong by one bit.

A cell names a sorter (mode, precision, dynamic, max_count), ascending `uploaded` values and per value the sorts to run.  The payload
width comes from `uploaded`, not from the list: an edge cell grows the sorter with set_uploaded_count (zero rows), keeps real centres
in [0, SPAN) and [u - SPAN, u) and sorts a host list of LIST_LEN entries drawn from both, u - 1 among them - the pass chain of a
16.7 M-splat scene in the time of a 24 k sort, and an oracle that reads only the listed rows of a host array of zeros."""
import numpy as np

import known_range_cases as kr
import sort_plan_cases as sc
import sort_plan_ref as ref

SPAN = 8192                                                # real centres at either end of an edge cell's sorter
LIST_LEN = 3 * 4096 * 2 + 1                                # (a chunk of the packed passes holds more than one tile)
SMALL_U = LIST_LEN                                         # an edge cell's first `uploaded` (a sort's counts are clamped to it)
SWEEP_N = (4097, LIST_LEN)
INT_PRECISIONS, FLOAT_PRECISIONS = tuple(range(10, 21)), tuple(range(10, 25))   # the Viewer's clamps (src/Viewer.js:208-210)
FRONT_PRECISIONS = (10, 13, 17, 20)                        # dynamic and precomputed sorters (float: and 24)
TOP = 1 << 24                                              # val_bits 24 | 25: the chunk-staged kernels' limit
BIG_U = (1 << 23) + 1                                      # the one large identity sort (precision 16)

# sorts: (kind, cull, precomputed).  full: the identity list; partial: its last third; perm: a permuted host list of u - 5;
# edge: LIST_LEN entries of [0, SPAN) and [u - SPAN, u)
FULL, PARTIAL, PERM, EDGE = "full", "partial", "perm", "edge"
INT_SWEEP = ((FULL, 0, 0), (FULL, 0, 0), (PARTIAL, 0, 0), (PERM, 0, 0), (FULL, 1, 0), (PERM, 1, 0))   # (twice: pass 0's slot is 3, then 0)
EDGE_SORTS = ((EDGE, 0, 0), (EDGE, 1, 0), (EDGE, 0, 1))
# float 24: three more cameras, two of them under the cull, so that some culled sort KEEPS a splat whose bucket is clamped (a
# clamp needs fp32 rounding to go up at the farthest splat: tests/test_sort_chains.py checks that it happens)
EDGE_SORTS_F24 = EDGE_SORTS + ((EDGE, 0, 0), (EDGE, 1, 0), (EDGE, 1, 0))

SWITCHES = {"GSPLAT_NO_SORT_CHUNK": "no_chunk", "GSPLAT_NO_SORT_PACK": "no_pack", "GSPLAT_NO_LDS_ATOMIC_RANK": None}


def pack_edge(precision):
    """The last `uploaded` at which pass 0 packs: precision - 8 + val_bits == 32."""
    return 1 << (40 - precision)


# (mode, precision) -> the `uploaded` values u whose pair (u, u + 1) flips pass 0's output or a pass's chunk staging
EDGES = {("int", 16): (TOP,), ("int", 10): (TOP,), ("float", 24): (pack_edge(24), TOP), ("float", 23): (pack_edge(23), TOP)}
EDGES.update({("int", p): (pack_edge(p),) for p in (17, 18, 19, 20)})
EDGES.update({("float", p): (pack_edge(p),) for p in (21, 22)})
# (float 23 at 2^24 + 1 is not one of the rows the matrix was asked for: KV32, then a packed word of 7 key bits above a 25-bit payload)


def _cell(name, mode, precision, steps, dynamic=False, data="gauss", dense=True, kind="sweep"):
    return dict(name=name, mode=mode, precision=precision, dynamic=dynamic, data=data, dense=dense, kind=kind,
                steps=tuple((u, tuple(sorts)) for u, sorts in steps), max_count=max(u for u, _ in steps))


def edge_cell(mode, precision, edges=None, sorts=EDGE_SORTS, kind="edge"):
    if (mode, precision) == ("float", 24) and sorts is EDGE_SORTS:
        sorts = EDGE_SORTS_F24
    us = [SMALL_U]
    for e in EDGES[(mode, precision)] if edges is None else edges:
        us += [e, e + 1]
    if (mode, precision) in (("int", 16), ("int", 10)) and edges is None:
        us.insert(1, (1 << 23) + 1)                        # val_bits 24 with payload bit 23 standing alone
    return _cell(f"edge_{mode}_p{precision}" + ("" if edges is None else "_" + "_".join(str(e) for e in edges)), mode, precision,
                 [(u, sorts) for u in us], dense=False, kind=kind)


def cells():
    out = []
    for n in SWEEP_N:
        for data in ("gauss", "grid"):
            out += [_cell(f"sweep_int_p{p}_{data}_{n}", "int", p, [(n, INT_SWEEP)], data=data) for p in INT_PRECISIONS]
            out += [_cell(f"sweep_float_p{p}_{data}_{n}", "float", p, [(n, [(FULL, 0, 0)])], data=data) for p in FLOAT_PRECISIONS]
        for p in FRONT_PRECISIONS + (24,):
            if p <= 20:
                out.append(_cell(f"front_dynamic_int_p{p}_{n}", "int", p, [(n, [(FULL, 0, 0), (PERM, 0, 0)])], dynamic=True, kind="front"))
                out.append(_cell(f"front_pre_int_p{p}_{n}", "int", p, [(n, [(FULL, 0, 1), (PERM, 0, 1)])], kind="front"))
            out.append(_cell(f"front_pre_float_p{p}_{n}", "float", p, [(n, [(FULL, 0, 1), (PERM, 0, 1)])], kind="front"))
    out += [edge_cell(mode, p) for mode, p in EDGES]
    out.append(_cell("big_identity_int_p16", "int", 16, [(BIG_U, [(FULL, 0, 0)])], dense=False, kind="big"))
    return out


def child_cells(switch):
    """What tests/tools/sort_chain_child.py runs under `switch`: the edge rows of integer 16, integer 20 and float 24; without
    packing also precisions 17 and 21 with payload bit 24 in their 32-bit key + value passes, and precision 10, whose 16-bit
    keys + values at 25 bits only the switch brings about (precision 16 does not pack there anyway)."""
    assert switch in SWITCHES
    out = [edge_cell("int", 16, kind="child"), edge_cell("int", 20, kind="child"), edge_cell("float", 24, kind="child")]
    if switch == "GSPLAT_NO_SORT_PACK":
        out += [edge_cell(mode, p, edges=(TOP,), sorts=EDGE_SORTS[:1], kind="child") for mode, p in (("int", 17), ("float", 21), ("int", 10))]
    return out


# ---------------------------------------------------------------------------------------------------
# the plan of a sort on the host model, and what of it the proof counts
# ---------------------------------------------------------------------------------------------------
def counts(u, kind):
    """(render_count, sort_count, host list?) of a sort of `kind` at `uploaded` = u."""
    if kind == FULL:
        return u, u, False
    if kind == PARTIAL:
        return u, u // 3, False
    if kind == PERM:
        return u - 5, u - 5, True
    return LIST_LEN, LIST_LEN, True


def plan_inputs(cell, u, sort, switch=None):
    kind, cull, pre = sort
    R, Rs, host = counts(u, kind)
    flags = (ref.SORT_INTEGER if cell["mode"] == "int" else 0) | (ref.SORT_DYNAMIC if cell["dynamic"] else 0)
    kw = dict(flags=flags, precision=cell["precision"], uploaded=u, render_count=R, sort_count=Rs, frustum_cull=cull,
              list=ref.LIST_HOST if host else ref.LIST_IDENTITY, precomputed=ref.PRE_HOST if pre else ref.PRE_NONE)
    if switch and SWITCHES[switch]:
        kw["sw_" + SWITCHES[switch]] = 1
    return sc.make_inputs(**kw)


def shape(pl):
    """A pass chain without its grids and slots: what each pass reads and writes, through which kernel, at which shift, and
    whether its histogram reads at val_bits (the packed words as plain keys; told from a shift that merely equals val_bits by
    the loader)."""
    return (pl["passes"],) + tuple((p["in"], p["out"], p["chunked"], p["shift"], int(p["in"] == ref.IN_PACKED and p["hist_shift"] == pl["val_bits"]),
                                    int(p["hist_shift"] == p["shift"])) for p in pl["pass"][:pl["passes"]])


def chain_key(inputs, plan_of=ref.sort_plan):
    """(shape, the switch that made it, whether the payload's top bit is bit 23, bit 24 or lower).  A switch that changes nothing
    of the plan (no chunk staging at 25 bits with or without it) does not count: the key is the plain one."""
    pl = plan_of(inputs)
    on = tuple(k for k in ("no_pack", "no_chunk") if inputs["sw"][k])
    if on:
        plain = dict(inputs, sw=dict(inputs["sw"], no_pack=0, no_chunk=0))
        if shape(plan_of(plain)) == shape(pl):
            on = ()
    return shape(pl), on, min(max(pl["val_bits"], 23), 25)


def reached(cell_list, switch=None):
    """{chain_key: [where]} over every sort of the cells."""
    out = {}
    for cell in cell_list:
        for u, sorts in cell["steps"]:
            for sort in sorts:
                out.setdefault(chain_key(plan_inputs(cell, u, sort, switch)), []).append((cell["name"], u, sort))
    return out


# ---------------------------------------------------------------------------------------------------
# the host's copy of a cell's sorter, and the arguments of its sorts
# ---------------------------------------------------------------------------------------------------
def _rng(*words):
    return np.random.default_rng([0x50C4] + [int(w) for w in words])


def _name_seed(cell):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(cell["name"]))


class Host:
    """What the cell's sorter holds, kept on the host: `advance(u)` yields the calls that bring the sorter to `uploaded` = u -
    ("rows", a, b, centres, scene indexes | None) for a `centers` message, ("fill", count) for set_uploaded_count - always
    appending, so that an integer sorter extends its extreme set and never rebuilds it from every row."""

    def __init__(self, cell):
        self.cell, self.uploaded = cell, 0
        self.use_int = cell["mode"] == "int"
        self.centers = np.zeros((cell["max_count"], 4), dtype=np.int32 if self.use_int else np.float32)
        self.scene = np.zeros(cell["max_count"], dtype=np.uint32) if cell["dynamic"] else None
        self.transforms = None
        if cell["dynamic"]:
            rng = _rng(_name_seed(cell), 7)
            t = np.tile(np.eye(4).reshape(16), (32, 1))
            for s in range(5):
                m = np.eye(4)
                m[:3, :3] += rng.normal(size=(3, 3)) * 0.2
                m[:3, 3] = rng.normal(size=3)
                t[s] = m.T.reshape(16)
            self.transforms = t.astype(np.float32)

    def _rows(self, a, b):
        cell, n = self.cell, b - a
        seed = _name_seed(cell) + 31 * a + b
        if cell["data"] == "grid":                         # many exactly equal keys (kat_cases' grid recipe)
            ci = np.empty((n, 4), dtype=np.int32)
            ci[:, :3] = _rng(seed).integers(-3, 4, size=(n, 3)) * 500
            ci[:, 3] = 1000
        else:
            ci = kr.gaussian_centers(n, seed=seed)
        rows = ci if self.use_int else np.concatenate([ci[:, :3].astype(np.float32) * np.float32(0.001), np.ones((n, 1), np.float32)], axis=1)
        scene = np.sort(_rng(seed, 1).integers(0, 5, size=n)).astype(np.uint32) if cell["dynamic"] else None
        self.centers[a:b] = rows
        if scene is not None:
            self.scene[a:b] = scene
        return ("rows", a, b, np.ascontiguousarray(rows), scene)

    def advance(self, u):
        assert self.uploaded < u <= self.cell["max_count"]
        ops, a = [], self.uploaded
        if not self.cell["dense"]:
            if a == 0 and u > 2 * SPAN:
                ops.append(self._rows(0, SPAN))
                a = SPAN
            if u - a > SPAN:
                ops.append(("fill", u - SPAN))
                a = u - SPAN
        ops.append(self._rows(a, u))
        self.uploaded = u
        return ops

    def pool(self, u):
        """The splats an edge list draws from: real centres, the lowest and the highest of the sorter."""
        return np.union1d(np.arange(min(SPAN, u), dtype=np.uint32), np.arange(max(u - SPAN, 0), u, dtype=np.uint32))

    def sort_args(self, u, sort, k=0):
        """dict(indexes | None, render_count, sort_count, cull, precomputed | None, mvp, listed): `listed` is the list the
        oracle sorts (the identity written out)."""
        kind, cull, pre = sort
        R, Rs, host = counts(u, kind)
        rng = _rng(_name_seed(self.cell), u, k)
        indexes = None
        if kind == PERM:
            indexes = rng.permutation(u).astype(np.uint32)[:R].copy()
        elif kind == EDGE:
            pool = self.pool(u)
            indexes = np.concatenate([pool, rng.choice(pool, LIST_LEN - len(pool))]).astype(np.uint32)
            rng.shuffle(indexes)
        listed = np.arange(u, dtype=np.uint32) if indexes is None else indexes
        precomputed = None
        if pre:                                            # one distance per uploaded splat; the listed ones matter
            precomputed = np.zeros(u, dtype=np.int32 if self.use_int else np.float32)
            m = len(listed) if kind == EDGE else u
            values = rng.integers(-2_000_000, 2_000_000, size=m) if self.use_int else rng.uniform(-30.0, 30.0, size=m)
            if kind == EDGE:
                precomputed[listed] = values
            else:
                precomputed[:] = values
        return dict(indexes=indexes, listed=listed, render_count=R, sort_count=Rs, cull=bool(cull), precomputed=precomputed,
                    mvp=kr.camera_mvp(k))

    def oracle(self, a):
        """(list, keys, buckets, (lo, hi), status) of the sort without its cull."""
        import oracle
        kw = dict(sort_count=a["sort_count"], render_count=a["render_count"], precision=self.cell["precision"], use_int=self.use_int,
                  dynamic=self.cell["dynamic"], precomputed=a["precomputed"], scene_indexes=self.scene, transforms=self.transforms)
        return oracle.sort_indexes(a["listed"], self.centers, a["mvp"], return_intermediates=True, **kw)


# ---------------------------------------------------------------------------------------------------
# one cell on the device
# ---------------------------------------------------------------------------------------------------
def run_cell(ctx, cell, cus, switch=None, log=None):
    """Every sort of the cell through a fresh SortWorker: the oracle bit for bit (known_range_cases.check_sort; a culled sort
    against oracle.culled_sort) and the executed plan against the host model, with the chain this module predicted.  Returns
    [(u, sort, clamped)]."""
    from gaussiansplats3d_amd import create_sort_worker
    host = Host(cell)
    use_int, precision = host.use_int, cell["precision"]
    w = create_sort_worker(ctx, cell["max_count"], True, True, use_int, cell["dynamic"], precision)
    done = []
    try:
        clean = 3
        for u, sorts in cell["steps"]:
            for op in host.advance(u):
                if op[0] == "fill":
                    w.set_uploaded_count(op[1])
                else:
                    w.post_message({"centers": op[3], "sceneIndexes": op[4], "range": {"from": op[1], "to": op[2] - 1, "count": op[2] - op[1]}})
            for k, sort in enumerate(sorts):
                a = host.sort_args(u, sort, k)
                what = f"{cell['name']} u {u} {sort}" + (f" {switch}" if switch else "")
                want_in = plan_inputs(cell, u, sort, switch)
                want = ref.sort_plan(want_in)
                known = bool(want["known_range"])
                w.set_frustum_cull(a["cull"])
                if a["cull"]:
                    clamped = check_culled(w, host, a, what)
                else:
                    kr.check_sort(w, host.centers, a["mvp"], kr.KNOWN if known else kr.OLD, sort_count=a["sort_count"],
                                  render_count=a["render_count"], indexes=a["indexes"], precision=precision, use_int=use_int,
                                  dynamic=cell["dynamic"], scene_indexes=host.scene, transforms=host.transforms,
                                  precomputed=a["precomputed"], uploaded=u, what=what)
                    clamped = int(w.last_stats()[0].clamped)
                arranged = {key: want_in[key] for key in ("flags", "precision", "uploaded", "frustum_cull", "list", "precomputed")}
                arranged.update({"sw_" + key: v for key, v in want_in["sw"].items()})
                if known:                                  # (compact or narrow by what the centres allow; wide above 16 bits)
                    arranged.update(clean_slot=clean, pass0_slot=clean, p0_in_narrow=int(precision <= 16), p0_skip_hist=1)
                else:
                    arranged.update(front=want["front"], pass0_slot=0, p0_skip_hist=0)
                _, pl = sc.check_executed(w, what, cu_count=cus, sort_count=a["sort_count"], render_count=a["render_count"],
                                          val_bits=want["val_bits"], known_range=int(known), passes=want["passes"], **arranged)
                assert shape(pl) == shape(want), f"{what}: ran {shape(pl)}, the matrix counts on {shape(want)}"
                clean = pl["next_clean_slot"]
                done.append((u, sort, clamped))
                if log:
                    log(f"{what}: chain {shape(pl)} val_bits {pl['val_bits']} clamped {clamped}")
    finally:
        w.terminate()
    return done


def check_culled(w, host, a, what):
    """A frustum-culled full sort: the plain sort's list without the dropped splats, the keep bit of every list position, the
    key range over every position.  Returns the clamp count."""
    import oracle
    R = a["render_count"]
    reply = w.post_message({"sort": {"modelViewProj": a["mvp"], "splatRenderCount": R, "splatSortCount": R, "indexesToSort": a["indexes"]}})
    _, keys, _, (lo, hi), _ = host.oracle(a)
    kept, keep = oracle.culled_sort(a["listed"], host.centers, a["mvp"], precision=host.cell["precision"], use_int=host.use_int)
    np.testing.assert_array_equal(w.keep_bits(R), keep, err_msg=what)
    stats = reply["stats"]
    assert stats.result_count == len(kept), what
    np.testing.assert_array_equal(reply["sortedIndexes"], kept, err_msg=what)
    assert (stats.key_min, stats.key_max) == (lo, hi), what
    # Only pass 0's histogram counts clamped buckets, and under a cull it decodes the kept positions alone (radix.hpp, hist_tiles:
    # `ok` needs ld.valid; the culling key kernel counts nothing): the oracle's clamps over the kept positions, and the status
    # that follows from them.
    clamps = oracle.count_clamped(keys[keep], lo, hi, host.cell["precision"])
    assert (int(stats.clamped), reply["status"]) == (clamps, 1 if clamps else 0), (what, int(stats.clamped), reply["status"], clamps)
    return clamps
