// sort_plan.hpp — the HOST POLICY of a depth sort (sort_plan.cpp; host only: no device, no context, no gs_sorter).
//
// What one gs_sorter_sort launches, decided in ONE function before anything is enqueued: what becomes of a pending gather, which
// front end keys the list, on which grids, which slot of group rows pass 0 owns, and per radix pass what it reads, what it writes,
// on which grid.  sorter.hip gathers the inputs, runs its refusals, calls plan_sort and then only acts on a `const SortPlan&`;
// tests/test_sort_plan.py holds plan_sort to a host model on a machine without a GPU (gs_debug_sort_plan).
// Both structs are plain 32-bit words (flags are 0 / 1), so the tests type them as they are and gs_sorter_debug_read(what = 5)
// hands out the executed pair word by word.
#pragma once
#include <stdint.h>

// ---------------------------------------------------------------------------------------------------
// geometry the policy shares with the kernels (radix.hpp, sorter.hip)
// ---------------------------------------------------------------------------------------------------
#ifndef RADIX_TILE_CFG
#define RADIX_TILE_CFG 4096
#endif
constexpr int RADIX_TILE = RADIX_TILE_CFG;                // keys per workgroup iteration
// Rows of a radix pass's offset table = the most workgroups (chunks) a pass may have.  The chunk-staged passes of the depth
// sort (radix.hpp) want <= 3 tiles per workgroup: 2048 rows cover 25 M keys.
#ifndef RADIX_MAX_BLOCKS_CFG
#define RADIX_MAX_BLOCKS_CFG 2048
#endif
constexpr int RADIX_MAX_BLOCKS = RADIX_MAX_BLOCKS_CFG;
// Grid cap of the tile-at-a-time scatter kernel.  Every workgroup starts by summing rows of the two-level offset table, so fewer,
// longer workgroups win: same-box A/B of the isolated C3 depth sort (r04a/b) 256: 0.0806 ms, 384: 0.0798, 512: 0.0733,
// 1024: 0.0822, 2048: 0.093 (r01e, whole frames: 2048: 0.498, 1024: 0.477, 512: 0.471, 384: 0.489, 256: 0.483).
#ifndef RADIX_TILE_GRID_CFG
#define RADIX_TILE_GRID_CFG 512
#endif
constexpr int RADIX_TILE_GRID = RADIX_TILE_GRID_CFG;
static_assert(RADIX_TILE_GRID <= RADIX_MAX_BLOCKS, "the tile kernel's grid needs a table row per workgroup");
constexpr int RADIX_MAX_PASSES = 4;
// the chunk-staged scatter (radix.hpp, k_radix_scatter_chunk): tiles a workgroup keeps in LDS at most, and how many workgroups
// (two per CU) the chunk length aims at
#ifndef CHUNK_TILES_CFG
#define CHUNK_TILES_CFG 3
#endif
constexpr int CHUNK_TILES = CHUNK_TILES_CFG;
#ifndef CHUNK_TARGET_BLOCKS_CFG
#define CHUNK_TARGET_BLOCKS_CFG 512
#endif
constexpr int CHUNK_TARGET_BLOCKS = CHUNK_TARGET_BLOCKS_CFG;

// n_upper: host-side upper bound of the element count.  The tile-at-a-time kernels' grid ...
inline uint32_t radix_grid_for(uint32_t n_upper) {
    uint32_t tiles = (n_upper + RADIX_TILE - 1) / RADIX_TILE;
    if (tiles < 1) tiles = 1;
    if (tiles <= (uint32_t)RADIX_TILE_GRID) return tiles;
    const uint32_t per = (tiles + RADIX_TILE_GRID - 1) / RADIX_TILE_GRID;
    return (tiles + per - 1) / per;
}
// ... and the chunk-staged kernel's.  0: too long for chunk-sized workgroups (the tile kernel takes it)
inline uint32_t radix_chunk_grid_for(uint32_t n_upper) {
    uint32_t tiles = (n_upper + RADIX_TILE - 1) / RADIX_TILE;
    if (tiles < 1) tiles = 1;
    uint32_t per = (tiles + CHUNK_TARGET_BLOCKS - 1) / CHUNK_TARGET_BLOCKS;
    if (per > (uint32_t)CHUNK_TILES) per = CHUNK_TILES;
    const uint32_t grid = (tiles + per - 1) / per;
    return grid <= (uint32_t)RADIX_MAX_BLOCKS ? grid : 0u;
}

// the visibility cull's front ends (sorter.hip): positions a workgroup takes per iteration / per turn
constexpr uint32_t VC_THREADS = 256, VC_SPAN = 1024;       // positions per workgroup iteration (4 per lane; 32 mask words)
constexpr uint32_t VC_WAVE_SPAN = 256;                     // positions per wave and span (4 per lane; 8 mask words)
constexpr uint32_t VC_UNROLL = 2;                          // spans per wave and turn (two turns' loads in flight: 2 x 8 x 16 bytes per lane)
constexpr uint32_t VC_TURN = VC_UNROLL * VC_WAVE_SPAN * (VC_THREADS / 64u);   // positions per workgroup and turn (2048)
constexpr uint32_t VC_DERIVE_SUBS = 4;                     // sub-workgroups per chunk of k_mask_derive_count
#ifndef GS_KEY_GRID_MULT
#define GS_KEY_GRID_MULT 2             // workgroups of k_depth_key<VEC4> per CU
#endif

// ---------------------------------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------------------------------
// The switches of sorter.hip (A/B runs and tests): read by sort_switches() there and nowhere else, once per process, at its first
// use (the tests and the soaks start a child process per setting).
struct SortSwitches {
    uint32_t tree_no_fuse;         // $GSPLAT_TREE_NO_FUSE: a planned gather is copied by tree.hip, never by the key kernel
    uint32_t vis_front;            // $GSPLAT_VIS_FRONT = stream (1) | compact (2): forces one front end of the visibility cull (0: unset)
    uint32_t no_pack;              // $GSPLAT_NO_SORT_PACK: the unpacked radix passes
    uint32_t no_chunk;             // $GSPLAT_NO_SORT_CHUNK: the tile-at-a-time scatter for packed passes
    uint32_t no_known_range;       // $GSPLAT_NO_KNOWN_RANGE: never k_depth_key_hist (and no extreme set is kept)
    uint32_t no_narrow_keys;       // $GSPLAT_NO_NARROW_KEYS: k_depth_key_hist stores the int32 depths whatever the precision
    uint32_t no_compact_centres;   // $GSPLAT_NO_COMPACT_CENTRES: k_depth_key_hist reads the int32 centre planes (and no 16-bit planes are kept)
};

// ---------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------
enum : uint32_t { SORT_LIST_IDENTITY = 0, SORT_LIST_HOST = 1, SORT_LIST_DEVICE = 2 };   // SortPlanIn::list
enum : uint32_t { SORT_PRE_NONE = 0, SORT_PRE_HOST = 1, SORT_PRE_DEVICE = 2 };          // SortPlanIn::precomputed

struct SortPlanIn {
    // the sorter
    uint32_t flags, precision, uploaded;       // GS_SORT_*; bits of a bucket; centres uploaded
    uint32_t frustum_cull, visibility_cull;
    uint32_t clean_slot;                       // the slot of group rows (0 or 3) the sort before left zeroed
    uint32_t pending_gather;                   // gs_tree_gather planned a gather whose lists this sorter has still to copy
    uint32_t pending_keep_zeroed;              // ... and zeroed this sorter's keep mask for a fused per-splat cull
    uint32_t extreme_current;                  // the (non-empty) extreme set covers the current centres
    uint32_t c16_current;                      // the 16-bit centre planes hold the current centres
    // the call
    uint32_t sort_count, render_count;         // as given (clamped to `uploaded` here)
    uint32_t list, precomputed;                // SORT_LIST_*, SORT_PRE_*
    uint32_t count_on_device;                  // the list's real length lives on the device (asynchronous gs_tree_gather)
    // the bound mesh (all 0: none)
    uint32_t mesh_map;                         // it hands out a position map for this sorter's centres (gs_mesh_payload_map)
    uint32_t mesh_uploaded;
    uint32_t mesh_strip;                       // its pending projection covers only some tile rows
    uint32_t mesh_lazy_mask;                   // ... and left the by-original-index mask to the sorter (gs_mesh::vis_orig_lazy)
    // the device
    uint32_t cu_count;
    // the exact key range over the extreme set (gs_key_range), evaluated when sort_wants_key_range() says so
    uint32_t range_ok;
    int32_t range_lo, range_hi;
    SortSwitches sw;
};

enum : uint32_t { SORT_GATHER_NONE = 0, SORT_GATHER_PLAIN = 1, SORT_GATHER_FUSED = 2 };   // SortPlan::gather
enum : uint32_t {                              // SortPlan::front: the first kernel(s) of the sort
    SORT_FRONT_NONE = 0,                       // nothing to sort (Rs == 0): nothing is launched
    SORT_FRONT_KNOWN_WIDE, SORT_FRONT_KNOWN_NARROW, SORT_FRONT_KNOWN_COMPACT,   // k_depth_key_hist<false> / <true> / <true, true>
    SORT_FRONT_TREE, SORT_FRONT_TREE_CULL,     // k_tree_copy_keys<false> / <true>
    SORT_FRONT_VIS_STREAM, SORT_FRONT_VIS_COMPACT,   // the visibility cull (with vis_derive / vis_map)
    SORT_FRONT_CULL_VEC4, SORT_FRONT_CULL_IDX, // k_depth_key_cull<true> / <false>
    SORT_FRONT_KEY_VEC4, SORT_FRONT_KEY_IDX,   // k_depth_key<true> / <false>
    SORT_FRONT_KINDS
};
enum : uint32_t { SORT_IN_DEPTH = 0, SORT_IN_PACKED = 1, SORT_IN_KEYS16 = 2, SORT_IN_KEYS32 = 3 };    // SortPass::in
enum : uint32_t { SORT_OUT_PACKED = 0, SORT_OUT_KV16 = 1, SORT_OUT_KV32 = 2, SORT_OUT_FINAL = 3 };    // SortPass::out
enum : uint32_t { SORT_COUNT_HOST = 0, SORT_COUNT_KEPT = 1, SORT_COUNT_LIST = 2 };                    // SortPlan::pass0_count

struct SortPass {
    uint32_t in;                   // the loader: the depth keys through a DepthLoader<in_cull, in_idx, in_narrow> (pass 0), the packed
    uint32_t in_cull, in_idx, in_narrow;   // word of the pass before, or its 16- / 32-bit key array + value array
    uint32_t out;                  // packed words (what is left of the key above the payload), keys + values, or the payloads alone
    uint32_t last;                 // the values go to the result (pass 0 of a one-pass sort still writes its 16-bit keys)
    uint32_t chunked;              // the chunk-staged scatter (radix.hpp)
    uint32_t shift, hist_shift;    // of the scatter's loader / the histogram's
    uint32_t slot;                 // its slot of group rows in RadixScratch::digit_total
    uint32_t grid;                 // workgroups of the histogram AND the scatter (a histogram row per workgroup)
    uint32_t skip_hist;            // the front end left this pass's histogram rows (on this grid, in this slot)
};

struct SortPlan {
    uint32_t R, Rs, sort_start;    // render count, sort count (both clamped), R - Rs
    uint32_t vis_cull;             // compact by the bound mesh's visibility mask, then sort the survivors
    uint32_t cull;                 // the frustum cull's keep-mask path; the visibility cull compacts instead
    uint32_t last_splat;           // uploaded - 1: list entries are clamped to it
    // The payload's range, not the list's: with a bound mesh a payload is perm[o], a position inside the mesh's slotted range,
    // which reaches mesh.uploaded - 1 even when fewer centres have reached this sorter (gs_mesh_payload_map allows
    // sorter.uploaded <= mesh.uploaded).  Sized from last_splat alone, the payload's top bits OR-ed into the key.
    uint32_t max_payload, val_bits;
    uint32_t gather;               // what becomes of a pending gather: SORT_GATHER_*
    uint32_t front;                // SORT_FRONT_*
    uint32_t vis_derive, vis_map;  // the visibility front end derives the mask itself / maps payloads through the mesh's position map
    // The front end's grids.  The known-range kernels have none of their own: they run on pass[0].grid, whose histogram rows
    // they write.  (The fused tree copy sizes its grid from the tree's leaves, where it is launched.)
    uint32_t front_grid, front_len;    // workgroups, and positions per workgroup where each owns a contiguous run
    uint32_t derive_grid, derive_len;  // chunks of k_mask_derive_count (launched VC_DERIVE_SUBS times as wide) and their length
    uint32_t counts_words;         // words of gs_sorter::chunk_counts the visibility front end needs
    uint32_t key_grid;             // SORT_FRONT_VIS_COMPACT: k_depth_key over the compacted list
    uint32_t known_range;          // the front end is one of SORT_FRONT_KNOWN_*
    int32_t range_lo, range_hi;    // ... with this exact key range (0, 0 otherwise)
    uint32_t pass0_slot;           // pass 0's slot of group rows
    uint32_t next_clean_slot;      // gs_sorter::clean_slot after this sort
    uint32_t own_payloads;         // the front end wrote the payloads itself (gs_sorter::pay_in): pass 0 neither gathers nor maps
    uint32_t pass0_count;          // where pass 0 reads the list's length: SORT_COUNT_*
    uint32_t pass0_publishes;      // a culling pass 0 compacts: it writes the result's length to SortFrame::kept
    uint32_t count_on_device;      // the later passes' element count and the result's length live in SortFrame::kept
    uint32_t passes;
    SortPass pass[RADIX_MAX_PASSES];
};

// The part of the plan gs_sorter_sort's refusals read, from the sorter and the call alone: the counts clamped to `uploaded`
// (Rs not yet to R: splatSortCount > splatRenderCount is refused) and which cull applies.
struct SortCounts { uint32_t R, Rs; bool vis_cull, cull; };
SortCounts sort_counts(const SortPlanIn& in);
// Whether plan_sort would take the known-range front end if `range_ok` were set: the caller evaluates the key range only then.
bool sort_wants_key_range(const SortPlanIn& in);
// Total: any input yields a plan whose grids and slots are within their tables (sort_count > render_count, which gs_sorter_sort
// refuses, is clamped; precision above 32 counts as 32; clean_slot other than 3 as 0; cu_count 0 as 1).
SortPlan plan_sort(const SortPlanIn& in);

// Debug entry for the tests (pure host; typed by tests/sort_plan_cases.py, not in the public header).
typedef SortPlanIn gs_sort_plan_debug_in;
typedef SortPlan gs_sort_plan_debug_out;
extern "C" int gs_debug_sort_plan(const gs_sort_plan_debug_in* in, gs_sort_plan_debug_out* out);   // 0, or -1 on a NULL argument
