"""The host policy of a depth sort restated in plain Python - the model tests/test_sort_plan.py and tests/test_gpu_sort_plan.py hold
csrc/sort_plan.cpp to.  It follows the sorter as it was BEFORE the plan existed, step by step and under that code's names: the
count clamps and culls of sort_check, the fused-gather rule of sort_stage_inputs, sort_known_range's eligibility, the branch order
of launch_front_end and launch_vis_cull_front with their grids, pass0_shape, and the loop of run_radix_passes, whose every branch
(one template instantiation each) is written down as the record {loader, output, chunked, shifts, slot, grid} it amounts to.

Inputs and outputs are dicts keyed like SortPlanIn / SortPlan (csrc/sort_plan.hpp); flags are 0 / 1."""

RADIX_TILE, RADIX_TILE_GRID, RADIX_MAX_BLOCKS, RADIX_MAX_PASSES = 4096, 512, 2048, 4
CHUNK_TILES, CHUNK_TARGET_BLOCKS = 3, 512
VC_SPAN, VC_TURN, DERIVE_SUBS, KEY_GRID_MULT = 1024, 2048, 4, 2
SORT_INTEGER, SORT_DYNAMIC = 1, 2
LIST_IDENTITY, LIST_HOST, LIST_DEVICE = 0, 1, 2
PRE_NONE, PRE_HOST, PRE_DEVICE = 0, 1, 2
GATHER_NONE, GATHER_PLAIN, GATHER_FUSED = 0, 1, 2
(FRONT_NONE, FRONT_KNOWN_WIDE, FRONT_KNOWN_NARROW, FRONT_KNOWN_COMPACT, FRONT_TREE, FRONT_TREE_CULL, FRONT_VIS_STREAM, FRONT_VIS_COMPACT,
 FRONT_CULL_VEC4, FRONT_CULL_IDX, FRONT_KEY_VEC4, FRONT_KEY_IDX) = range(12)
IN_DEPTH, IN_PACKED, IN_KEYS16, IN_KEYS32 = 0, 1, 2, 3
OUT_PACKED, OUT_KV16, OUT_KV32, OUT_FINAL = 0, 1, 2, 3
COUNT_HOST, COUNT_KEPT, COUNT_LIST = 0, 1, 2
U32 = 0xFFFFFFFF

PASS_FIELDS = ["in", "in_cull", "in_idx", "in_narrow", "out", "last", "chunked", "shift", "hist_shift", "slot", "grid", "skip_hist"]
PLAN_FIELDS = ["R", "Rs", "sort_start", "vis_cull", "cull", "last_splat", "max_payload", "val_bits", "gather", "front", "vis_derive",
               "vis_map", "front_grid", "front_len", "derive_grid", "derive_len", "counts_words", "key_grid", "known_range", "range_lo",
               "range_hi", "pass0_slot", "next_clean_slot", "own_payloads", "pass0_count", "pass0_publishes", "count_on_device", "passes"]


def radix_grid_for(n):
    tiles = max(((n + RADIX_TILE - 1) & U32) // RADIX_TILE, 1)
    if tiles <= RADIX_TILE_GRID:
        return tiles
    per = (tiles + RADIX_TILE_GRID - 1) // RADIX_TILE_GRID
    return (tiles + per - 1) // per


def radix_chunk_grid_for(n):
    tiles = max(((n + RADIX_TILE - 1) & U32) // RADIX_TILE, 1)
    per = min((tiles + CHUNK_TARGET_BLOCKS - 1) // CHUNK_TARGET_BLOCKS, CHUNK_TILES)
    grid = (tiles + per - 1) // per
    return grid if grid <= RADIX_MAX_BLOCKS else 0


def grid_for(n, per_block, cap):
    return min(max((n + per_block - 1) // per_block, 1), cap)


def chunk_grid(cus, R, unit):
    units = (R + unit - 1) // unit
    grid = min(units, cus * 2)
    return grid, ((units + grid - 1) // grid) * unit


def _pass(**kw):
    rec = dict.fromkeys(PASS_FIELDS, 0)
    rec.update(kw)
    return rec


def sort_plan(i):
    """The plan of one gs_sorter_sort whose refusals have passed (sort_count <= render_count after the clamp)."""
    sw = i["sw"]
    pl = dict.fromkeys(PLAN_FIELDS, 0)
    integer, dynamic, pre = bool(i["flags"] & SORT_INTEGER), bool(i["flags"] & SORT_DYNAMIC), i["precomputed"] != PRE_NONE
    device_list, has_list, count_dev = i["list"] == LIST_DEVICE, i["list"] != LIST_IDENTITY, bool(i["count_on_device"])
    precision, uploaded = i["precision"], i["uploaded"]
    # sort_check
    R, Rs = min(i["render_count"], uploaded), min(i["sort_count"], uploaded)
    assert Rs <= R, "splatSortCount > splatRenderCount is refused before anything is planned"
    vis_cull = bool(i["visibility_cull"]) and not count_dev
    cull = bool(i["frustum_cull"]) and not vis_cull
    sort_start = R - Rs
    last_splat = uploaded - 1 if uploaded else 0
    max_payload = last_splat
    if i["mesh_map"] and i["mesh_uploaded"] and i["mesh_uploaded"] - 1 > max_payload:
        max_payload = i["mesh_uploaded"] - 1
    val_bits = 1
    while val_bits < 32 and (max_payload >> val_bits):
        val_bits += 1
    pl.update(R=R, Rs=Rs, sort_start=sort_start, vis_cull=int(vis_cull), cull=int(cull), last_splat=last_splat, max_payload=max_payload,
              val_bits=val_bits, next_clean_slot=i["clean_slot"])
    # sort_stage_inputs: a planned gather
    fused_tree = False
    if device_list and i["pending_gather"]:
        fused_tree = (not sw["tree_no_fuse"] and Rs == R and Rs > 0 and not dynamic and not pre and not vis_cull
                      and (not cull or bool(i["pending_keep_zeroed"])))
        pl["gather"] = GATHER_FUSED if fused_tree else GATHER_PLAIN
    if Rs == 0:
        pl["passes"] = 0
        pl["pass"] = [_pass() for _ in range(RADIX_MAX_PASSES)]
        return pl
    # launch_front_end
    cus = i["cu_count"]
    mode_int = integer and not dynamic and not pre
    vec4 = mode_int and not has_list
    known = not (sw["no_known_range"] or not mode_int or has_list or fused_tree or vis_cull or cull or count_dev or sort_start != 0
                 or R != uploaded or R == 0)
    known = known and bool(i["extreme_current"]) and bool(i["range_ok"])
    pass0_slot = i["clean_slot"] if known else 0
    pl["pass0_slot"], pl["next_clean_slot"] = pass0_slot, (0 if pass0_slot == 3 else 3)
    narrow = known and precision <= 16 and not sw["no_narrow_keys"]
    compact = narrow and not sw["no_compact_centres"] and bool(i["c16_current"])
    vis_front = False
    if known:
        pl.update(front=FRONT_KNOWN_COMPACT if compact else FRONT_KNOWN_NARROW if narrow else FRONT_KNOWN_WIDE, known_range=1,
                  range_lo=i["range_lo"], range_hi=i["range_hi"])
    elif fused_tree:
        pl["front"] = FRONT_TREE_CULL if cull else FRONT_TREE
    elif vis_cull:                                          # launch_vis_cull_front
        lazy = bool(i["mesh_lazy_mask"])
        dg = chunk_grid(cus, R, VC_TURN * DERIVE_SUBS)
        vis_front = (sw["vis_front"] == 1) if sw["vis_front"] else not i["mesh_strip"]
        pl.update(vis_derive=int(lazy), vis_map=int(bool(i["mesh_map"])))
        if lazy:
            pl.update(derive_grid=dg[0], derive_len=dg[1])
        if vis_front:
            wg = dg if lazy else chunk_grid(cus, R, VC_TURN)
            pl.update(front=FRONT_VIS_STREAM, front_grid=wg[0], front_len=wg[1], counts_words=wg[0] * DERIVE_SUBS)
        else:
            cg = chunk_grid(cus, R, VC_SPAN)
            pl.update(front=FRONT_VIS_COMPACT, front_grid=cg[0], front_len=cg[1],
                      counts_words=max(dg[0] * DERIVE_SUBS if lazy else 0, cg[0]), key_grid=grid_for(Rs, 256 * 4, cus * 2))
    elif cull:
        pl.update(front=FRONT_CULL_VEC4 if vec4 else FRONT_CULL_IDX,
                  front_grid=grid_for(Rs, 256 * 16, cus * 2) if vec4 else grid_for(Rs, 256 * 4, cus * 4))
    else:
        pl.update(front=FRONT_KEY_VEC4 if vec4 else FRONT_KEY_IDX,
                  front_grid=grid_for(Rs, 256 * 16, cus * KEY_GRID_MULT) if vec4 else grid_for(Rs, 256 * 4, cus * 2))
    # pass0_shape
    chunked = not sw["no_chunk"] and val_bits <= 24 and radix_chunk_grid_for(Rs) != 0
    pack0 = precision > 8 and not sw["no_pack"] and (precision - 8) + val_bits <= 32
    grid0 = radix_chunk_grid_for(Rs) if (pack0 and chunked) else radix_grid_for(Rs)
    # run_radix_passes
    own_payloads = fused_tree or vis_front
    idx_dev = has_list or vis_cull                          # (the visibility cull's front end leaves its list in idx_in)
    has_idx = own_payloads or idx_dev
    passes = (precision + 7) // 8
    wide = precision > 16
    pl.update(own_payloads=int(own_payloads), passes=passes, count_on_device=int(cull or vis_cull or count_dev),
              pass0_count=COUNT_KEPT if vis_cull else COUNT_LIST if count_dev else COUNT_HOST, pass0_publishes=int(cull))
    recs, in_packed = [], False
    for p in range(passes):
        last = p + 1 == passes
        left = precision - 8 * (p + 1)
        pack = not last and not sw["no_pack"] and left + val_bits <= 32
        shift = 0 if in_packed else 8 * p
        tile_grid = radix_grid_for(Rs)
        if p == 0:
            assert pack == pack0, "pass0_shape and the loop decide pass 0's packing alike"
            loader = dict(in_narrow=1) if narrow else dict(in_cull=int(cull), in_idx=int(has_idx))
            if pack and chunked:
                out, ch, grid = OUT_PACKED, 1, radix_chunk_grid_for(Rs)
            elif pack:
                out, ch, grid = OUT_PACKED, 0, tile_grid
            elif wide and not narrow:
                out, ch, grid = OUT_KV32, 0, tile_grid
            else:
                out, ch, grid = OUT_KV16, 0, tile_grid
            assert grid == grid0, "the key kernel's grid is pass 0's"
            recs.append(_pass(out=out, last=int(last), chunked=ch, shift=shift, hist_shift=shift, slot=pass0_slot, grid=grid,
                              skip_hist=int(known), **{"in": IN_DEPTH}, **loader))
        elif in_packed:
            out = OUT_FINAL if last else OUT_PACKED
            recs.append(_pass(out=out, last=int(last), chunked=int(chunked), shift=0, hist_shift=val_bits, slot=p,
                              grid=radix_chunk_grid_for(Rs) if chunked else tile_grid, **{"in": IN_PACKED}))
        elif wide:
            out = OUT_FINAL if last else OUT_PACKED if pack else OUT_KV32
            recs.append(_pass(out=out, last=int(last), shift=shift, hist_shift=shift, slot=p, grid=tile_grid, **{"in": IN_KEYS32}))
        else:
            assert last, "16-bit keys: two passes"
            recs.append(_pass(out=OUT_FINAL, last=1, shift=shift, hist_shift=shift, slot=p, grid=tile_grid, **{"in": IN_KEYS16}))
        in_packed = in_packed or pack
    pl["pass"] = recs + [_pass() for _ in range(RADIX_MAX_PASSES - passes)]
    return pl
