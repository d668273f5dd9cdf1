"""The cases of tests/test_sort_plan.py: inputs of the library's pure-host debug entry gs_debug_sort_plan (csrc/sort_plan.cpp), typed
here, and what each case is there to show.

`python tests/sort_plan_cases.py dump FILE` writes the cases' input structs one after the other: what the stand-alone sanitizer
program tests/tools/sort_plan_fuzz.cpp reads."""
import ctypes as C
import sys

import sort_plan_ref as ref

SWITCHES = ["tree_no_fuse", "vis_front", "no_pack", "no_chunk", "no_known_range", "no_narrow_keys", "no_compact_centres"]


class Switches(C.Structure):                               # SortSwitches (csrc/sort_plan.hpp)
    _fields_ = [(name, C.c_uint32) for name in SWITCHES]


IN_WORDS = ["flags", "precision", "uploaded", "frustum_cull", "visibility_cull", "clean_slot", "pending_gather", "pending_keep_zeroed",
            "extreme_current", "c16_current", "sort_count", "render_count", "list", "precomputed", "count_on_device", "mesh_map",
            "mesh_uploaded", "mesh_strip", "mesh_lazy_mask", "cu_count", "range_ok"]


class PlanIn(C.Structure):                                 # SortPlanIn = gs_sort_plan_debug_in
    _fields_ = [(name, C.c_uint32) for name in IN_WORDS] + [("range_lo", C.c_int32), ("range_hi", C.c_int32), ("sw", Switches)]


class Pass(C.Structure):                                   # SortPass
    _fields_ = [(name, C.c_uint32) for name in ref.PASS_FIELDS]


class PlanOut(C.Structure):                                # SortPlan = gs_sort_plan_debug_out
    _fields_ = [(name, C.c_int32 if name in ("range_lo", "range_hi") else C.c_uint32) for name in ref.PLAN_FIELDS] + \
               [("pass", Pass * ref.RADIX_MAX_PASSES)]


def to_struct(i):
    s = PlanIn()
    for name in IN_WORDS + ["range_lo", "range_hi"]:
        setattr(s, name, i[name])
    for name in SWITCHES:
        setattr(s.sw, name, i["sw"][name])
    return s


def in_from_struct(s):
    i = {name: getattr(s, name) for name in IN_WORDS + ["range_lo", "range_hi"]}
    i["sw"] = {name: getattr(s.sw, name) for name in SWITCHES}
    return i


def out_from_struct(o):
    pl = {name: getattr(o, name) for name in ref.PLAN_FIELDS}
    pl["pass"] = [{name: getattr(getattr(o, "pass")[p], name) for name in ref.PASS_FIELDS} for p in range(ref.RADIX_MAX_PASSES)]
    return pl


def differences(got, want):
    """{field: (got, want)} over two plans."""
    d = {k: (got[k], want[k]) for k in ref.PLAN_FIELDS if got[k] != want[k]}
    for p, (a, b) in enumerate(zip(got["pass"], want["pass"])):
        d.update({f"pass[{p}].{k}": (a[k], b[k]) for k in ref.PASS_FIELDS if a[k] != b[k]})
    return d


def executed(worker):
    """(inputs, plan) of the worker's last sort as it ran: gs_sorter_debug_read(what = 5)."""
    nin, nout = C.sizeof(PlanIn) // 4, C.sizeof(PlanOut) // 4
    words = worker.debug_read(5, nin + nout)
    return (in_from_struct(PlanIn.from_buffer_copy(words[:nin].tobytes())), out_from_struct(PlanOut.from_buffer_copy(words[nin:].tobytes())))


def check_executed(worker, what="", **arranged):
    """The last sort ran on the inputs the test arranged (sw_*: switches) and on the plan the model makes of them; arranged keys
    that name plan fields (front, gather, p0_out ..) are held to the plan.  Returns (inputs, plan)."""
    i, pl = executed(worker)
    for k, v in arranged.items():
        if k.startswith("sw_"):
            got = i["sw"][k[3:]]
        elif k[0] == "p" and k[1].isdigit():
            got = pl["pass"][int(k[1])][k[3:]]
        elif k.startswith("plan_"):                           # (a name both structs have: the plan's)
            got = pl[k[5:]]
        elif k in i:
            got = i[k]
        else:
            got = pl[k]
        assert got == v, f"{what}: {k} is {got}, arranged {v}"
    want = ref.sort_plan(i)
    assert not differences(pl, want), f"{what}: {differences(pl, want)}"
    return i, pl


def make_inputs(**kw):
    """The Viewer's default sort: every uploaded centre of a static integer sorter, precision 16, a current extreme set and range,
    current 16-bit planes, no mesh, no switch - the compact known-range front end.  Keyword arguments replace fields; sw_* set
    switches; n = ... sets uploaded, sort_count and render_count at once."""
    i = dict(flags=ref.SORT_INTEGER, precision=16, uploaded=100000, frustum_cull=0, visibility_cull=0, clean_slot=3, pending_gather=0,
             pending_keep_zeroed=0, extreme_current=1, c16_current=1, sort_count=100000, render_count=100000, list=ref.LIST_IDENTITY,
             precomputed=ref.PRE_NONE, count_on_device=0, mesh_map=0, mesh_uploaded=0, mesh_strip=0, mesh_lazy_mask=0, cu_count=256,
             range_ok=1, range_lo=-123456, range_hi=654321, sw=dict.fromkeys(SWITCHES, 0))
    if "n" in kw:
        n = kw.pop("n")
        i.update(uploaded=n, sort_count=n, render_count=n)
    for k, v in kw.items():
        if k.startswith("sw_"):
            assert k[3:] in i["sw"], k
            i["sw"][k[3:]] = v
        else:
            assert k in i, k
            i[k] = v
    return i


def _p(pl, p):
    return pl["pass"][p]


def cases():
    """[(name, inputs, check)]: check(plan) asserts what the case is named for."""
    R = ref
    out = []

    def case(name, check, **kw):
        out.append((name, make_inputs(**kw), check))

    def expect(**want):
        def check(pl):
            for k, v in want.items():
                if k.startswith("p") and k[1].isdigit():
                    got = _p(pl, int(k[1]))[k[3:]]
                else:
                    got = pl[k]
                assert got == v, (k, got, v)
        return check

    # --- the default, and clean_slot ---
    case("default_compact_known_range", expect(front=R.FRONT_KNOWN_COMPACT, known_range=1, pass0_slot=3, next_clean_slot=0, passes=2,
                                               p0_skip_hist=1, p0_in_narrow=1, p0_out=R.OUT_PACKED, p0_chunked=1, p1_in=R.IN_PACKED,
                                               p1_out=R.OUT_FINAL, p1_slot=1, p1_hist_shift=17))
    case("clean_slot_0", expect(pass0_slot=0, next_clean_slot=3), clean_slot=0)
    case("old_path_uses_slot_0_and_leaves_3", expect(known_range=0, pass0_slot=0, next_clean_slot=3, p0_skip_hist=0), clean_slot=3,
         sw_no_known_range=1)
    case("old_path_from_clean_slot_0", expect(pass0_slot=0, next_clean_slot=3), clean_slot=0, sw_no_known_range=1)
    # --- precision x payload width: left + val_bits at 32 and at 33 ---
    case("precision_8_one_pass", expect(passes=1, p0_out=R.OUT_KV16, p0_last=1, p0_chunked=0), precision=8)
    case("precision_9_left_1", expect(passes=2, p0_out=R.OUT_PACKED, p1_out=R.OUT_FINAL), precision=9)
    case("precision_9_val_bits_31_packs", expect(val_bits=31, p0_out=R.OUT_PACKED, p0_chunked=0, p1_in=R.IN_PACKED, p1_chunked=0),
         precision=9, n=1 << 31)
    case("precision_9_val_bits_32_does_not", expect(val_bits=32, p0_out=R.OUT_KV16, p1_in=R.IN_KEYS16), precision=9, n=(1 << 31) + 1)
    case("precision_16_2p23_packs", expect(val_bits=23, p0_out=R.OUT_PACKED, p0_chunked=1), n=1 << 23)
    case("precision_16_2p24_val_24_left_8_is_32", expect(val_bits=24, p0_out=R.OUT_PACKED, p0_chunked=1, p1_chunked=1), n=1 << 24)
    case("precision_16_2p24_plus_1_val_25_is_33", expect(val_bits=25, p0_out=R.OUT_KV16, p0_chunked=0, p1_in=R.IN_KEYS16, p1_out=R.OUT_FINAL),
         n=(1 << 24) + 1)
    case("precision_17_val_15_left_9_packs_at_once", expect(passes=3, val_bits=15, p0_out=R.OUT_PACKED, p1_out=R.OUT_PACKED, p2_out=R.OUT_FINAL,
                                                           p1_shift=0, p2_shift=0, p2_slot=2), precision=17, n=1 << 15)
    case("precision_17_val_24_packs_in_pass_1", expect(front=R.FRONT_KNOWN_WIDE, val_bits=24, p0_out=R.OUT_KV32, p1_in=R.IN_KEYS32,
                                                      p1_out=R.OUT_PACKED, p1_chunked=0, p1_shift=8, p2_in=R.IN_PACKED, p2_chunked=1,
                                                      p2_shift=0, p2_hist_shift=24), precision=17, n=1 << 24)
    case("precision_20_val_20_left_12_is_32", expect(val_bits=20, p0_out=R.OUT_PACKED), precision=20, n=1 << 20)
    case("precision_20_val_21_left_12_is_33", expect(val_bits=21, p0_out=R.OUT_KV32, p1_out=R.OUT_PACKED), precision=20, n=(1 << 20) + 1)
    case("precision_24_float", expect(passes=3, front=R.FRONT_KEY_IDX, val_bits=16, p0_out=R.OUT_PACKED, p2_out=R.OUT_FINAL), precision=24, flags=0,
         n=1 << 16)
    case("precision_24_val_17_is_33", expect(val_bits=17, p0_out=R.OUT_KV32, p1_out=R.OUT_PACKED, p2_in=R.IN_PACKED), precision=24, flags=0,
         n=(1 << 16) + 1)
    case("precision_24_val_25_never_packs", expect(val_bits=25, p0_out=R.OUT_KV32, p1_out=R.OUT_KV32, p2_in=R.IN_KEYS32, p2_out=R.OUT_FINAL,
                                                  p2_shift=16), precision=24, flags=0, n=(1 << 24) + 1)
    case("mesh_larger_than_the_sorter_sizes_the_payload", expect(last_splat=999, max_payload=(1 << 24), val_bits=25, p0_out=R.OUT_KV16), n=1000,
         mesh_map=1, mesh_uploaded=(1 << 24) + 1)
    case("mesh_without_a_map_does_not", expect(max_payload=999, val_bits=10), n=1000, mesh_map=0, mesh_uploaded=(1 << 24) + 1)
    # --- chunked: val_bits 24 against 25, the list's length ---
    case("val_bits_24_chunked", expect(val_bits=24, p0_chunked=1, p1_chunked=1), precision=10, n=1 << 24)
    case("val_bits_25_packed_not_chunked", expect(val_bits=25, p0_out=R.OUT_PACKED, p0_chunked=0, p1_chunked=0), precision=10, n=(1 << 24) + 1)
    case("empty_list", expect(front=R.FRONT_NONE, passes=0, next_clean_slot=3, count_on_device=0), sort_count=0, render_count=0)
    case("empty_sorter", expect(front=R.FRONT_NONE, R=0, Rs=0, last_splat=0, val_bits=1), n=0)
    case("one_splat", expect(front=R.FRONT_KNOWN_COMPACT, p0_grid=1, val_bits=1), n=1)
    for n, grid in ((R.RADIX_TILE - 1, 1), (R.RADIX_TILE, 1), (R.RADIX_TILE + 1, 2)):
        case(f"tile_boundary_{n}", expect(p0_grid=grid, p1_grid=grid), n=n)
    for n, grid in ((512 * 4096 - 1, 512), (512 * 4096, 512), (512 * 4096 + 1, 257)):
        case(f"chunk_target_boundary_{n}", expect(p0_chunked=1, p0_grid=grid), n=n)
    case("tile_grid_past_512_tiles", expect(p0_chunked=0, p0_grid=257), n=512 * 4096 + 1, sw_no_chunk=1)
    # (the first length for which radix_chunk_grid_for is 0 needs a 25-bit payload, which rules the chunk-staged kernel out by itself:
    # on both sides of it the tile kernel runs, on its own grid)
    first_unchunked = next(n for n in range(2048 * 3 * 4096, 2048 * 3 * 4096 + 2) if ref.radix_chunk_grid_for(n) == 0)
    case("last_length_radix_chunk_grid_for_is_not_0", expect(val_bits=25, p0_chunked=0, p0_grid=512), precision=10,
         n=first_unchunked - 1)
    case("first_length_radix_chunk_grid_for_is_0", expect(val_bits=25, p0_chunked=0, p0_grid=ref.radix_grid_for(first_unchunked)), precision=10,
         n=first_unchunked)
    # --- every switch on its own ---
    case("switch_no_pack", expect(p0_out=R.OUT_KV16, p0_chunked=0, p1_in=R.IN_KEYS16), sw_no_pack=1)
    case("switch_no_pack_wide", expect(p0_out=R.OUT_KV32, p1_out=R.OUT_KV32, p2_out=R.OUT_FINAL), precision=20, sw_no_pack=1)
    case("switch_no_chunk", expect(p0_out=R.OUT_PACKED, p0_chunked=0, p1_chunked=0), sw_no_chunk=1)
    case("switch_no_known_range", expect(front=R.FRONT_KEY_VEC4, known_range=0, range_lo=0, range_hi=0), sw_no_known_range=1)
    case("switch_no_narrow_keys", expect(front=R.FRONT_KNOWN_WIDE, p0_in_narrow=0), sw_no_narrow_keys=1)
    case("switch_no_compact_centres_narrow_without_compact", expect(front=R.FRONT_KNOWN_NARROW, p0_in_narrow=1), sw_no_compact_centres=1)
    case("stale_planes_narrow_without_compact", expect(front=R.FRONT_KNOWN_NARROW), c16_current=0)
    case("switch_tree_no_fuse", expect(gather=R.GATHER_PLAIN, front=R.FRONT_KEY_IDX), list=R.LIST_DEVICE, pending_gather=1, sw_tree_no_fuse=1)
    # --- every reason that keeps a sort off the known-range path ---
    old = dict(known_range=0, p0_skip_hist=0, pass0_slot=0)
    case("off_float", expect(front=R.FRONT_KEY_IDX, **old), flags=0)
    case("off_dynamic", expect(front=R.FRONT_KEY_IDX, **old), flags=R.SORT_INTEGER | R.SORT_DYNAMIC)
    case("off_precomputed_host", expect(front=R.FRONT_KEY_IDX, **old), precomputed=R.PRE_HOST)
    case("off_precomputed_device", expect(front=R.FRONT_KEY_IDX, **old), precomputed=R.PRE_DEVICE)
    case("off_host_list", expect(front=R.FRONT_KEY_IDX, p0_in_idx=1, **old), list=R.LIST_HOST)
    case("off_device_list", expect(front=R.FRONT_KEY_IDX, gather=R.GATHER_NONE, p0_in_idx=1, **old), list=R.LIST_DEVICE)
    case("off_pending_tree", expect(front=R.FRONT_TREE, gather=R.GATHER_FUSED, own_payloads=1, p0_in_idx=1, **old), list=R.LIST_DEVICE, pending_gather=1)
    case("off_device_length_list", expect(front=R.FRONT_TREE, count_on_device=1, pass0_count=R.COUNT_LIST, **old), list=R.LIST_DEVICE,
         pending_gather=1, count_on_device=1)
    case("off_frustum_cull", expect(front=R.FRONT_CULL_VEC4, cull=1, count_on_device=1, pass0_publishes=1, p0_in_cull=1, p0_in_idx=0, **old),
         frustum_cull=1)
    case("off_visibility_cull", expect(front=R.FRONT_VIS_STREAM, vis_cull=1, cull=0, pass0_count=R.COUNT_KEPT, **old), visibility_cull=1, mesh_map=1,
         mesh_uploaded=100000)
    case("off_partial_sort", expect(front=R.FRONT_KEY_VEC4, sort_start=40000, **old), sort_count=60000)
    case("off_render_below_uploaded", expect(front=R.FRONT_KEY_VEC4, R=99999, **old), sort_count=99999, render_count=99999)
    case("counts_clamped_to_uploaded_stay_on", expect(front=R.FRONT_KNOWN_COMPACT, R=100000, Rs=100000), sort_count=1 << 30, render_count=1 << 31)
    case("off_stale_extreme_set", expect(front=R.FRONT_KEY_VEC4, **old), extreme_current=0)
    case("off_range_not_ok", expect(front=R.FRONT_KEY_VEC4, range_lo=0, range_hi=0, **old), range_ok=0)
    # --- the other front ends ---
    case("frustum_cull_on_a_list", expect(front=R.FRONT_CULL_IDX, p0_in_cull=1, p0_in_idx=1, front_grid=98), frustum_cull=1, list=R.LIST_HOST)
    case("frustum_cull_float", expect(front=R.FRONT_CULL_IDX, p0_in_idx=0), frustum_cull=1, flags=0)
    case("both_culls_visibility_wins", expect(vis_cull=1, cull=0, pass0_publishes=0), frustum_cull=1, visibility_cull=1)
    case("visibility_cull_gives_way_to_a_device_length_list", expect(vis_cull=0, cull=1, front=R.FRONT_TREE_CULL), frustum_cull=1, visibility_cull=1,
         list=R.LIST_DEVICE, pending_gather=1, pending_keep_zeroed=1, count_on_device=1)
    case("key_grids_capped_by_the_cus", expect(front=R.FRONT_KEY_VEC4, front_grid=16), sw_no_known_range=1, cu_count=8)
    # --- fused tree: refused by each of its conditions ---
    tree = dict(list=R.LIST_DEVICE, pending_gather=1)
    plain = dict(gather=R.GATHER_PLAIN, own_payloads=0)
    case("tree_fused_with_cull", expect(gather=R.GATHER_FUSED, front=R.FRONT_TREE_CULL, p0_in_cull=1, p0_in_idx=1), frustum_cull=1,
         pending_keep_zeroed=1, **tree)
    case("tree_plain_keep_mask_not_zeroed", expect(front=R.FRONT_CULL_IDX, **plain), frustum_cull=1, pending_keep_zeroed=0, **tree)
    case("tree_plain_partial_sort", expect(front=R.FRONT_KEY_IDX, **plain), sort_count=5, **tree)
    case("tree_plain_empty", expect(front=R.FRONT_NONE, **plain), sort_count=0, render_count=0, **tree)
    case("tree_plain_dynamic", expect(front=R.FRONT_KEY_IDX, **plain), flags=R.SORT_INTEGER | R.SORT_DYNAMIC, **tree)
    case("tree_plain_precomputed", expect(front=R.FRONT_KEY_IDX, **plain), precomputed=R.PRE_HOST, **tree)
    case("tree_plain_visibility_cull", expect(vis_cull=1, front=R.FRONT_VIS_STREAM, gather=R.GATHER_PLAIN), visibility_cull=1, **tree)
    case("tree_float_fuses", expect(gather=R.GATHER_FUSED, front=R.FRONT_TREE), flags=0, **tree)
    case("no_pending_gather_no_action", expect(gather=R.GATHER_NONE), list=R.LIST_DEVICE)
    case("pending_gather_left_alone_by_an_identity_sort", expect(gather=R.GATHER_NONE, front=R.FRONT_KNOWN_COMPACT), pending_gather=1)
    # --- visibility front end: strip / full frame, forced either way, with and without the lazy mask ---
    vis = dict(visibility_cull=1, mesh_map=1, mesh_uploaded=100000)
    case("vis_full_frame_streams", expect(front=R.FRONT_VIS_STREAM, vis_derive=0, vis_map=1, own_payloads=1, front_grid=49, front_len=2048,
                                         counts_words=196, key_grid=0, derive_grid=0, p0_in_idx=1), **vis)
    case("vis_strip_compacts", expect(front=R.FRONT_VIS_COMPACT, own_payloads=0, front_grid=98, front_len=1024, counts_words=98, key_grid=98,
                                     p0_in_idx=1), mesh_strip=1, **vis)
    case("vis_full_frame_lazy_mask", expect(front=R.FRONT_VIS_STREAM, vis_derive=1, derive_grid=13, derive_len=8192, front_grid=13, front_len=8192,
                                           counts_words=52), mesh_lazy_mask=1, **vis)
    case("vis_forced_stream_on_a_strip", expect(front=R.FRONT_VIS_STREAM), mesh_strip=1, sw_vis_front=1, **vis)
    case("vis_forced_compact_on_a_full_frame", expect(front=R.FRONT_VIS_COMPACT, vis_derive=0), sw_vis_front=2, **vis)
    case("vis_forced_compact_lazy_mask_derives_first", expect(front=R.FRONT_VIS_COMPACT, vis_derive=1, derive_grid=13, counts_words=98), sw_vis_front=2,
         mesh_lazy_mask=1, **vis)
    case("vis_forced_stream_lazy", expect(front=R.FRONT_VIS_STREAM, vis_derive=1), sw_vis_front=1, mesh_lazy_mask=1, mesh_strip=1, **vis)
    case("vis_without_a_map", expect(front=R.FRONT_VIS_STREAM, vis_map=0, max_payload=99999), visibility_cull=1, mesh_map=0, mesh_uploaded=100000)
    case("vis_few_cus_long_chunks", expect(front_grid=4, front_len=26624), cu_count=2, **vis)
    return out


def clean_slot_sequence():
    """Front ends of consecutive sorts of one sorter: (inputs without clean_slot, pass 0's slot, clean_slot afterwards)."""
    known, oldp, empty = {}, dict(sw_no_known_range=1), dict(sort_count=0, render_count=0)
    return [(known, 3, 0), (known, 0, 3), (oldp, 0, 3), (known, 3, 0), (oldp, 0, 3), (oldp, 0, 3), (known, 3, 0), (empty, 0, 0), (known, 0, 3),
            (empty, 0, 3), (known, 3, 0)]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        with open(sys.argv[2], "wb") as f:
            for _, inputs, _ in cases():
                f.write(bytes(to_struct(inputs)))
        print(f"{len(cases())} cases, {C.sizeof(PlanIn)} bytes each")
    else:
        print("usage: sort_plan_cases.py dump FILE")
