// sort_plan.cpp — the host policy of a depth sort (sort_plan.hpp): everything gs_sorter_sort decides before it launches.
#include "sort_plan.hpp"

#include <algorithm>

#include "../../include/gsplat_hip.h"

static inline uint32_t grid_for(uint32_t n, uint32_t per_block, uint32_t cap) {
    uint32_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return g > cap ? cap : g;
}

// The cut of R > 0 positions for a streaming front end: a workgroup owns a contiguous run of whole units, at most two
// workgroups per CU.
struct ChunkGrid { uint32_t grid, len; };
static ChunkGrid chunk_grid(uint32_t cus, uint32_t R, uint32_t unit) {
    const uint32_t units = (R + unit - 1u) / unit;
    const uint32_t grid = units < cus * 2u ? units : cus * 2u;
    return {grid, ((units + grid - 1u) / grid) * unit};
}

// What the counts, the flags and the bound mesh make of the call (SortWorker.js:100-101 clamps both counts to the uploaded
// splat count), and what becomes of a pending gather.
SortCounts sort_counts(const SortPlanIn& in) {
    SortCounts n;
    n.R = std::min(in.render_count, in.uploaded);
    n.Rs = std::min(in.sort_count, in.uploaded);
    n.vis_cull = in.visibility_cull && !in.count_on_device;    // (sorts the identity list: not combinable with a gathered one)
    n.cull = in.frustum_cull && !n.vis_cull;
    return n;
}

static void plan_call(const SortPlanIn& in, SortPlan& pl) {
    const SortCounts n = sort_counts(in);
    pl.R = n.R;
    pl.Rs = std::min(n.Rs, n.R);
    pl.sort_start = pl.R - pl.Rs;
    pl.vis_cull = n.vis_cull;
    pl.cull = n.cull;
    pl.last_splat = in.uploaded ? in.uploaded - 1u : 0u;
    pl.max_payload = pl.last_splat;
    if (in.mesh_map && in.mesh_uploaded && in.mesh_uploaded - 1u > pl.max_payload) pl.max_payload = in.mesh_uploaded - 1u;
    pl.val_bits = 1;
    while (pl.val_bits < 32u && (pl.max_payload >> pl.val_bits)) pl.val_bits++;
    // A gather that was only planned (tree.hip) is copied by this sort: by its key kernel when it is a full sort of a static scene
    // (and, with the frustum cull, the gather zeroed the keep mask the copy ORs into), else by tree.hip's plain copy.
    pl.gather = SORT_GATHER_NONE;
    if (in.list == SORT_LIST_DEVICE && in.pending_gather) {
        const bool fused = !in.sw.tree_no_fuse && pl.Rs == pl.R && pl.Rs > 0 && !(in.flags & GS_SORT_DYNAMIC) && !in.precomputed && !pl.vis_cull &&
                           (!pl.cull || in.pending_keep_zeroed);
        pl.gather = fused ? SORT_GATHER_FUSED : SORT_GATHER_PLAIN;
    }
}

// The exact key range of a sort is known before anything is launched (gs_key_range: min / max of im . c over the extreme set)
// only for the plain full sort of every uploaded centre in static integer mode.  Everything else keeps the key kernel +
// histogram path.
static bool known_range_eligible(const SortPlanIn& in, const SortPlan& pl) {
    const bool static_int = in.flags == GS_SORT_INTEGER && !in.precomputed;
    return !in.sw.no_known_range && static_int && in.list == SORT_LIST_IDENTITY && !pl.vis_cull && !pl.cull && !in.count_on_device &&
           pl.sort_start == 0u && pl.R == in.uploaded && pl.R != 0u && in.extreme_current;
}

bool sort_wants_key_range(const SortPlanIn& in) {
    SortPlan pl = {};
    plan_call(in, pl);
    return known_range_eligible(in, pl);
}

// The first kernel(s) of the sort: keys, min / max, the housekeeping - one kind per kernel family - and their grids.
static void plan_front(const SortPlanIn& in, SortPlan& pl) {
    const uint32_t cus = std::max(in.cu_count, 1u);
    const bool vec4 = (in.flags & GS_SORT_INTEGER) && !(in.flags & GS_SORT_DYNAMIC) && !in.precomputed && in.list == SORT_LIST_IDENTITY;
    pl.known_range = known_range_eligible(in, pl) && in.range_ok;
    if (pl.known_range) {
        pl.range_lo = in.range_lo;
        pl.range_hi = in.range_hi;
        // a radix key of <= 16 bits travels as 16 bits (the same lo and hi decide the buckets, whichever kernel applies them) ...
        const bool narrow = in.precision <= 16u && !in.sw.no_narrow_keys;
        // ... and then its centres come from the 16-bit offset planes, where they hold the centres as they are now
        const bool compact = narrow && !in.sw.no_compact_centres && in.c16_current;
        pl.front = compact ? SORT_FRONT_KNOWN_COMPACT : narrow ? SORT_FRONT_KNOWN_NARROW : SORT_FRONT_KNOWN_WIDE;
    } else if (pl.gather == SORT_GATHER_FUSED) {
        pl.front = pl.cull ? SORT_FRONT_TREE_CULL : SORT_FRONT_TREE;
    } else if (pl.vis_cull) {
        // Two front ends, chosen by what the vertex stage drew.  A full frame keeps a large part of the scene (C3: a quarter):
        // the streaming front end keys the survivors on the way (N = 1 frame 0.285 -> 0.270 ms, r05k).  A rank's strip keeps
        // a few per cent: round 4's chain - a 12-byte-per-splat min / max pass, a compaction of the mask, and centre gathers
        // for the few survivors - is the cheaper one there (C3 rank 4 of 8: 0.116 vs 0.126 ms, same box), because the streaming
        // kernel also reads the payload table (+4 bytes per splat) and runs at 2.8 TB/s where the pure reduction reaches 4.
        // $GSPLAT_VIS_FRONT = stream | compact forces one (A/B and tests).
        const bool stream = in.sw.vis_front ? in.sw.vis_front == 1u : !in.mesh_strip;
        pl.front = stream ? SORT_FRONT_VIS_STREAM : SORT_FRONT_VIS_COMPACT;
        // The projection left the by-original-index mask to the sorter: k_mask_derive_count builds it from the storage-order
        // mask through the payload map (a chunk of it is a whole number of VC_DERIVE_SUBS x turns: one piece per sub-workgroup)
        pl.vis_derive = in.mesh_lazy_mask != 0u;
        pl.vis_map = in.mesh_map != 0u;
        const ChunkGrid dg = chunk_grid(cus, pl.R, VC_TURN * VC_DERIVE_SUBS);
        if (pl.vis_derive) { pl.derive_grid = dg.grid; pl.derive_len = dg.len; }
        if (stream) {
            // one contiguous run of positions per workgroup, walked in turns of VC_TURN (two workgroups per CU)
            const ChunkGrid wg = pl.vis_derive ? dg : chunk_grid(cus, pl.R, VC_TURN);
            pl.front_grid = wg.grid; pl.front_len = wg.len;
            pl.counts_words = wg.grid * VC_DERIVE_SUBS;
        } else {
            const ChunkGrid cg = chunk_grid(cus, pl.R, VC_SPAN);
            pl.front_grid = cg.grid; pl.front_len = cg.len;
            pl.counts_words = std::max(pl.vis_derive ? dg.grid * VC_DERIVE_SUBS : 0u, cg.grid);
            pl.key_grid = grid_for(pl.Rs, 256 * 4, cus * 2);
        }
    } else if (pl.cull) {
        pl.front = vec4 ? SORT_FRONT_CULL_VEC4 : SORT_FRONT_CULL_IDX;
        pl.front_grid = vec4 ? grid_for(pl.Rs, 256 * 16, cus * 2) : grid_for(pl.Rs, 256 * 4, cus * 4);
    } else {
        pl.front = vec4 ? SORT_FRONT_KEY_VEC4 : SORT_FRONT_KEY_IDX;
        pl.front_grid = vec4 ? grid_for(pl.Rs, 256 * 16, cus * GS_KEY_GRID_MULT) : grid_for(pl.Rs, 256 * 4, cus * 2);
    }
    // every other front end zeroes all four slots and the passes use slots 0 .. 2; the known-range kernel zeroes all but its own
    pl.pass0_slot = pl.known_range && in.clean_slot == 3u ? 3u : 0u;
    pl.next_clean_slot = pl.pass0_slot == 3u ? 0u : 3u;
    // the fused copy / the cull's streaming front end wrote the payloads themselves
    pl.own_payloads = pl.gather == SORT_GATHER_FUSED || pl.front == SORT_FRONT_VIS_STREAM;
}

// The radix passes over key' = range - 1 - bucket of the reversed list: pass 0 reads the keys through a DepthLoader.
// What travels between the passes: after pass p the key still holds precision - 8 (p + 1) bits.  When those fit above the
// payload in one 32-bit word (payloads are splat positions < uploaded: 23 bits at 5.8 M splats, 24 at 16 M, so the default
// 16-bit buckets always do below 2^24 splats) the pass writes that word instead of a key array and a value array
// (radix.hpp PACK_OUT); otherwise 16- or 32-bit keys + values, and a later pass packs as soon as it can.
static void plan_passes(const SortPlanIn& in, SortPlan& pl) {
    const uint32_t precision = std::min(in.precision, 32u);
    const bool narrow = pl.front == SORT_FRONT_KNOWN_NARROW || pl.front == SORT_FRONT_KNOWN_COMPACT;
    const bool wide = precision > 16u;
    // Packed passes stage a whole chunk in LDS (radix.hpp) when the list is short enough for <= CHUNK_TILES tiles per
    // workgroup and the payload leaves 8 bits for the digit beside it in the last pass's staging word.
    const uint32_t chunk_grid = radix_chunk_grid_for(pl.Rs);
    const bool chunked = !in.sw.no_chunk && pl.val_bits <= 24u && chunk_grid != 0u;
    // after a culling pass 0 the element count is the device-resident kept count
    pl.count_on_device = pl.cull || pl.vis_cull || in.count_on_device;
    pl.pass0_count = pl.vis_cull ? SORT_COUNT_KEPT : in.count_on_device ? SORT_COUNT_LIST : SORT_COUNT_HOST;
    pl.pass0_publishes = pl.cull;
    pl.passes = (precision + 7u) / 8u;
    bool in_packed = false;                                // the pass before packed
    for (uint32_t p = 0; p < pl.passes; p++) {
        SortPass& ps = pl.pass[p];
        const bool last = p + 1u == pl.passes;
        const uint32_t left = precision - std::min(precision, 8u * (p + 1u));    // key bits after this pass
        const bool pack = !last && (in_packed || (!in.sw.no_pack && left + pl.val_bits <= 32u));
        ps.last = last;
        ps.slot = p == 0u ? pl.pass0_slot : p;
        ps.shift = ps.hist_shift = in_packed ? 0u : 8u * p;
        if (p == 0u) {
            ps.in = SORT_IN_DEPTH;
            ps.in_narrow = narrow;                         // (a known-range sort: the identity list, no cull)
            ps.in_cull = !narrow && pl.cull;
            ps.in_idx = !narrow && (pl.own_payloads || in.list != SORT_LIST_IDENTITY || pl.vis_cull);
            ps.out = pack ? SORT_OUT_PACKED : wide ? SORT_OUT_KV32 : SORT_OUT_KV16;
            ps.chunked = pack && chunked;
            ps.skip_hist = pl.known_range;
        } else if (in_packed) {
            ps.in = SORT_IN_PACKED;
            ps.hist_shift = pl.val_bits;                   // the histogram reads the packed words as plain 32-bit keys
            ps.out = last ? SORT_OUT_FINAL : SORT_OUT_PACKED;
            ps.chunked = chunked;
        } else {
            ps.in = wide ? SORT_IN_KEYS32 : SORT_IN_KEYS16;
            ps.out = last ? SORT_OUT_FINAL : (pack && wide) ? SORT_OUT_PACKED : wide ? SORT_OUT_KV32 : SORT_OUT_KV16;
        }
        ps.grid = ps.chunked ? chunk_grid : radix_grid_for(pl.Rs);
        in_packed = in_packed || ps.out == SORT_OUT_PACKED;
    }
}

SortPlan plan_sort(const SortPlanIn& in) {
    SortPlan pl = {};
    plan_call(in, pl);
    pl.next_clean_slot = in.clean_slot;
    if (pl.Rs > 0u) {
        plan_front(in, pl);
        plan_passes(in, pl);
    }
    return pl;
}

extern "C" int gs_debug_sort_plan(const gs_sort_plan_debug_in* in, gs_sort_plan_debug_out* out) {
    if (!in || !out) return -1;
    *out = plan_sort(*in);
    return 0;
}
