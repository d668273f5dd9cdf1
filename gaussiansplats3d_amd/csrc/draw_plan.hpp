// draw_plan.hpp — the HOST POLICY of a draw (draw_plan.cpp; host only: no device, no context, no gs_mesh).
//
// What a draw decides from the draw before it: where the vertex stage runs its block test, how large the list bins are, whether the
// previous draw's statistics order the blend's bins (and shifted by how many bins), whether the deep pass runs, and where and how
// many of its workgroups sit in the blend's launch.  None of it changes a pixel.  Plain structs and free functions, every input by
// value: the launch code (mesh.hip, project.hip, tile_bin.hip, tile_blend.hip) fills the inputs and acts on the result, and
// tests/test_draw_plan.py holds every function to a host model on a machine without a GPU (gs_debug_draw_plan).
#pragma once
#include <stdint.h>

#include "../../include/gsplat_hip.h"

// ---------------------------------------------------------------------------------------------------
// geometry the policy shares with the kernels
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t GS_BIN_SHIFT = 1;                       // a blend workgroup owns a bin of 2x2 tiles of 16 px = 32x32 px
constexpr uint32_t GS_BIN = GS_TILE << GS_BIN_SHIFT;
// The entry lists are per LIST BIN of (16 << GS_LIST_SHIFT) px.  The blend reads only the head of a list before its pixels
// saturate (C3: the first 256 of ~2900 entries per 32-px bin, tools/blend_profile.py), so emitting and sorting per-32-px
// entries mostly produced entries nobody read.  128-px list bins cut the entries 3.7x and their sort to ONE 8-bit pass at
// 1080p (15 x 9 = 135 lists); a blend workgroup scans its parent list and keeps what touches its own 32-px block.
// That only pays when splats are large enough to share lists: a scene of many tiny splats (C4: 16 M splats of ~1.5 tiles)
// gains no entries and makes every blend workgroup scan 16 bins' worth of them, so the size is chosen per mesh from the
// statistics of its last measured draw (gs_mesh::list_shift): 128 px when a visible splat covers >= 3 tiles, else 32 px.
constexpr uint32_t GS_LIST_SHIFT_LARGE = 3;                // 128-px list bins
constexpr uint32_t GS_LIST_SHIFT_SMALL = GS_BIN_SHIFT;     // 32-px list bins = one list per blend workgroup
constexpr float GS_LIST_TILES_PER_SPLAT = 3.0f;
// ... and 256- / 512-px list bins when splats are larger still: what matters is the list bin's area against the splat's (a bin
// scans the entries of its whole list): 128 px at 10 tiles per splat (C3) is 6x, and lists of 36x (C2 at 256 px) or 100x (C3T at
// 512 px) make the blend scan itself to a standstill (r04 tools/list_shift_ab.py: C2 0.281 -> 0.372 -> 0.947 ms at 128 / 256 / 512
// px, C3T 0.598 -> 0.906 -> 2.20).  So the size follows the splats at <= ~12x: 256 px from 21 tiles per visible splat, 512 px
// from 80 (an 8K frame of the garden stand-in covers 101: entries 5.96 M -> 2.19 M, its 2040 lists become 135 and its two-pass
// entry sort one pass (0.082 -> 0.022 ms), the binner 0.091 -> 0.056 ms, the blend scans 24 % more (0.654 -> 0.686 ms): frame
// 0.903 -> 0.837 ms; a rank of eight 0.267 -> 0.228 ms).
constexpr uint32_t GS_LIST_SHIFT_BIG = 4, GS_LIST_SHIFT_HUGE = 5;          // 256- / 512-px list bins
constexpr float GS_LIST_TILES_PER_SPLAT_BIG = 21.0f, GS_LIST_TILES_PER_SPLAT_HUGE = 80.0f;
constexpr uint32_t GS_DEEP_MAX_BINS = 512;                 // bins the deep pass takes at most (gs_internal.hpp: the deep pass)

// ---------------------------------------------------------------------------------------------------
// the mapped host words (gs_mesh::mirror_host): written by every draw's k_bin_emit, read by the host without a synchronisation
// ---------------------------------------------------------------------------------------------------
// [0..3] one 16-byte store {serial, overflow, entries lo, hi}: the entry buffer's verdict (mesh.hip, mesh_heal_overflow)
constexpr uint32_t GS_MIRROR_SERIAL = 0, GS_MIRROR_OVERFLOW = 1, GS_MIRROR_ENTRIES_LO = 2, GS_MIRROR_ENTRIES_HI = 3;
// [4] bins over the deep pass's trigger (0: none), [5] their share of the last walk in 1 / 1024: the schedule job's verdict
constexpr uint32_t GS_MIRROR_DEEP_CANDIDATES = 4, GS_MIRROR_DEEP_SHARE = 5;
// [8..11] one 16-byte store {serial, visible splats, 16-px tiles they touch lo, hi}: how much of the scene is in view
constexpr uint32_t GS_MIRROR_VIEW_SERIAL = 8, GS_MIRROR_VISIBLE = 9, GS_MIRROR_TILES16_LO = 10, GS_MIRROR_TILES16_HI = 11;
constexpr uint32_t GS_MIRROR_WORDS = 16;                   // allocated (64 bytes)
static_assert(GS_MIRROR_SERIAL % 4 == 0 && GS_MIRROR_OVERFLOW == GS_MIRROR_SERIAL + 1 && GS_MIRROR_ENTRIES_LO == GS_MIRROR_SERIAL + 2 &&
              GS_MIRROR_ENTRIES_HI == GS_MIRROR_SERIAL + 3, "k_bin_emit writes the verdict as one aligned 16-byte store");
static_assert(GS_MIRROR_VIEW_SERIAL % 4 == 0 && GS_MIRROR_VISIBLE == GS_MIRROR_VIEW_SERIAL + 1 && GS_MIRROR_TILES16_LO == GS_MIRROR_VIEW_SERIAL + 2 &&
              GS_MIRROR_TILES16_HI == GS_MIRROR_VIEW_SERIAL + 3, "k_bin_emit writes the view share as one aligned 16-byte store");

// One snapshot of the words.  Each 16-byte group lands together but a newer draw may be writing it: its serial is read again after
// the group, and a group whose serial changed (or, for the view share, is still 0: no draw yet) is "not valid, look again next time".
struct DrawFeedback {
    bool entries_valid;        // serial / overflow / entries belong to one draw
    uint32_t serial;
    bool overflow;
    uint64_t entries;          // entries that draw needed
    uint32_t deep_candidates;  // single words: whatever the last schedule job that has arrived left
    uint32_t deep_share;
    bool view_valid;           // view_serial / visible / tiles16 belong to one draw
    uint32_t view_serial, visible;
    uint64_t tiles16;
};
DrawFeedback read_feedback(const volatile uint32_t* mirror);   // (nullptr: nothing valid, no candidates)

// ---------------------------------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------------------------------
// The switches of the draw path (A/B runs and tests): read by draw_switches() (mesh.hip) and nowhere else, fetched once per
// gs_mesh_render / gs_mesh_project and handed down.  (What a mesh or a context reads when it is created lives on gs_mesh / gs_context.)
struct DrawSwitches {
    // read once per process, at its first draw (the tests and the soaks start a child process per setting):
    uint32_t deep_min;             // $GSPLAT_DEEP_MIN: (splat, quadrant) pairs a bin's previous draw walked before the deep pass takes it (4 * GS_CHUNK)
    uint32_t deep_factor;          // $GSPLAT_DEEP_FACTOR: ... and that many times the mean bin (3)
    uint32_t pool_slots;           // $GSPLAT_POOL_SLOTS: chunk partials the per-bin kernel may close, at most GS_POOL_SLOTS
    bool no_lazy_mask;             // $GSPLAT_NO_LAZY_MASK: gs_mesh_project writes the by-original-index mask itself, never the bound sorter
    // read on every draw (tests, tools and the bench set them inside a running process):
    bool no_blend_order;           // $GSPLAT_NO_BLEND_ORDER: no schedule job, the blend's bins in row-major order
    float order_motion;            // $GSPLAT_ORDER_MOTION: parallax, in screen heights, up to which the previous draw's order is taken (0.045)
    bool no_stat_shift;            // $GSPLAT_NO_STAT_SHIFT: the previous draw's statistics are read unshifted
    bool blend_order_stale;        // $GSPLAT_BLEND_ORDER_STALE: order from whatever draw came before (rounds 2-5)
    bool deep_row_major_on_motion; // $GSPLAT_DEEP_ROW_MAJOR_ON_MOTION: a deep-pass draw of a moved camera drops the order as well
    bool no_async_list_bins;       // $GSPLAT_NO_ASYNC_LIST_BINS: the list-bin size follows statistics reads only, not the mapped words
    bool deep_units_last;          // $GSPLAT_DEEP_UNITS_LAST: the deep pass's workgroups behind every bin, all of them
    bool no_compact_bin_word;      // $GSPLAT_NO_COMPACT_BIN_WORD: the binner's look-up word is the 8-byte one on every frame
};

// ---------------------------------------------------------------------------------------------------
// the list bins, the entry room, the block test
// ---------------------------------------------------------------------------------------------------
// List-bin size (a shift: a list bin is (16 << shift) px) of the following draws, from what a draw saw: `current`, the 16-px tiles
// its visible splats touch, and how many splats were visible (0: nothing to go by, `current` stays).
uint32_t adapt_list_shift(uint32_t current, uint64_t tiles16, uint32_t visible);

// Entry slots to allocate for a draw that needs `need`: an eighth of head room and 1024.  (Every caller clamps or refuses at
// 2^31 - 1 itself.)
inline uint64_t entry_room(uint64_t need) { return need + need / 8 + 1024; }

// Where the vertex stage runs its block test: 1 = k_block_test + k_project, 0 = the test in every workgroup, 2 = no test.
// measured_visible / measured_count: of the mesh's last measured full-frame draw (count 0: nothing measured); strip: this draw
// covers only some tile rows; block_cull: ProjectParams::block_cull; the two switches: $GSPLAT_NO_BLOCK_LIST, $GSPLAT_BLOCK_TEST_ALWAYS.
int block_test_mode(uint32_t measured_visible, uint32_t measured_count, bool strip, bool block_cull, bool no_block_list, bool block_test_always);

// Which look-up word (bin_word.hpp) the vertex stage leaves for the binner: the 4-byte one where its origin fields hold every tile
// of the frame, the 8-byte one beyond 256 tiles in either direction (an 8K frame) and under $GSPLAT_NO_COMPACT_BIN_WORD.
bool narrow_bin_word(uint32_t tiles_x, uint32_t tiles_y, const DrawSwitches& sw);

// ---------------------------------------------------------------------------------------------------
// k_bin_emit's work units (host and device: the kernel and gs_debug_live_units run the same two functions)
// ---------------------------------------------------------------------------------------------------
// k_bin_count leaves cnt[b] compacted splats in slice b (one binning workgroup's part of the walk, room for per * 256); k_bin_emit
// expands them in batches of GS_EMIT_BATCH.  Only the batches that hold a splat are dealt - at C3 a slice keeps a quarter of its
// positions, so three of four (slice, batch) pairs are empty and, dealt round-robin by pair, the empty ones land on the same
// workgroups every time.  Live unit l of a draw is batch l - first[b] of the slice b with first[b] <= l < first[b + 1], where first
// is the exclusive prefix of ceil(cnt / 256) over the slices and first[slices] = the draw's live units.  Workgroup wg of wgs takes
// l = wg, wg + wgs, ...: the near end of the walk stays spread over the grid.
// One word per slice, so the kernel's LDS holds what it held: first[b] in 24 bits (a sorted list is < 2^32 positions, and fewer than
// 2^24 batches since its array is < 4 GiB) | (cnt[b] - 1) & 255 above: a slice's batches are full but for its last one.
#if defined(__HIP__)       // (the attributes spelled out: draw_plan.cpp includes no HIP header)
#define GS_PLAN_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GS_PLAN_FN inline
#endif
constexpr uint32_t GS_EMIT_BATCH = 256;
constexpr uint32_t GS_LIVE_FIRST_MASK = 0x00FFFFFFu;
GS_PLAN_FN uint32_t live_batches(uint32_t cnt) { return (cnt + GS_EMIT_BATCH - 1u) / GS_EMIT_BATCH; }
GS_PLAN_FN uint32_t live_unit_word(uint32_t first, uint32_t cnt) { return (first & GS_LIVE_FIRST_MASK) | (((cnt - 1u) & 255u) << 24); }
struct LiveUnit {
    uint32_t slice, batch;         // batch `batch` of slice `slice` ...
    uint32_t count;                // ... which holds this many splats (1 .. 256)
};
// Unit l, once its slice is known: `word` is the slice's, next_first the first unit of the slice after it (the draw's live units
// behind the last slice).
GS_PLAN_FN LiveUnit live_unit_of(uint32_t slice, uint32_t word, uint32_t next_first, uint32_t l) {
    const uint32_t first = word & GS_LIVE_FIRST_MASK;
    LiveUnit u;
    u.slice = slice;
    u.batch = l - first;
    u.count = u.batch + 1u < next_first - first ? GS_EMIT_BATCH : (word >> 24) + 1u;
    return u;
}
// word_at(b): the word of slice b < slices; total: the draw's live units; l < total.  The unit's slice is the LAST one whose first
// is <= l: never an empty one (an empty slice's successor has the same first).  A binary search here; k_bin_emit finds the same
// slice with two ballots of a wave over its LDS (tile_bin.hip, live_unit_find_wave: eleven dependent LDS reads per unit were a
// third of a unit's time) and decodes it with live_unit_of as well.
template <class WordAt>
GS_PLAN_FN LiveUnit live_unit_find(WordAt word_at, uint32_t slices, uint32_t total, uint32_t l) {
    uint32_t lo = 0u, hi = slices;                         // first[lo] <= l < first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((word_at(mid) & GS_LIVE_FIRST_MASK) <= l) lo = mid;
        else hi = mid;
    }
    return live_unit_of(lo, word_at(lo), hi < slices ? (word_at(hi) & GS_LIVE_FIRST_MASK) : total, l);
}

// ---------------------------------------------------------------------------------------------------
// the blend schedule and the deep pass
// ---------------------------------------------------------------------------------------------------
// A draw's camera and what else of its geometry the statistics of its blend depend on
struct PlanView {
    float view[16], proj[16];      // column-major modelView and projection (ProjectParams)
    float width, height;
    uint32_t count, list_shift;
};
// What gs_mesh::blend_stats describes: the bins of the last draw that blended any, and the view of the last draw enqueued.  Set in
// ONE place, once a draw's blend is enqueued (mesh.hip, mesh_draw_once).
struct StatsOf {
    bool valid;                    // a draw has been enqueued: `view` is set
    uint32_t bins, row_begin, width_px;   // the bins the statistics were written for (0: none yet) ...
    uint32_t draw_mode;            // ... and the draw mode (GS_DRAW_*) that wrote them: they schedule a later draw of the SAME mode only
    PlanView view;
};
struct ScheduleInputs {
    StatsOf stats;                 // what the statistics describe
    PlanView now;                  // this draw
    uint32_t bins_x, bin_row_begin, bin_row_end;   // its 32-px bins
    uint32_t block_cull;           // ProjectParams::block_cull (0: per-scene transforms, the scene's centre says nothing)
    uint32_t draw_mode;            // GS_DRAW_*
    uint32_t draw_serial;          // of the draw BEFORE this one (gs_mesh::draw_serial before it is advanced)
    bool no_deep;                  // $GSPLAT_NO_DEEP / gs_mesh_set_deep_pass(0)
    double centre_sum[3];          // over every finite centre uploaded ...
    uint64_t centre_n;             // ... and how many
    DrawFeedback feedback;         // the mapped words as this draw found them
    DrawSwitches sw;
};
struct SchedulePlan {
    uint32_t blend_bins;           // this draw's 32-px bins
    bool order_ok;                 // the statistics are of these bins, in this draw mode: a schedule job could read them
    bool same_view;                // ... and of this view, or one close enough (the motion gate)
    int32_t sx, sy;                // this draw's bin (bx, by) shows what the previous draw's bin (bx - sx, by - sy) showed
    bool order_wg;                 // k_bin_emit runs the schedule job (one extra workgroup)
    bool order_taken;              // the blend visits its bins in the job's order (else row-major)
    bool deep_pass;                // this draw runs the deep pass
    uint32_t deep_min, deep_factor;   // what the job is given
};
SchedulePlan plan_schedule(const ScheduleInputs& in);

// Where the deep pass's workgroups sit in the blend's launch of `bins` per-bin workgroups, and how many there are; occupancy: blend
// workgroups a CU holds.
struct DeepUnits { uint32_t unit_at, unit_wgs; };
DeepUnits place_deep_units(const SchedulePlan& plan, uint32_t bins, uint32_t cu_count, uint32_t occupancy, const DrawFeedback& feedback,
                           const DrawSwitches& sw);

// ---------------------------------------------------------------------------------------------------
// Debug entry for the tests (pure host; typed by tests/test_draw_plan.py, not in the public header): the five functions on plain
// inputs.  Flags are uint32 (0 / 1).
struct gs_draw_plan_debug_in {
    double centre_sum[3];
    uint64_t centre_n;
    uint64_t tiles16;              // adapt_list_shift(list_current, tiles16, visible)
    uint64_t need;                 // entry_room(need)
    uint32_t mirror[GS_MIRROR_WORDS];   // read_feedback: the words as this draw finds them
    // what the statistics describe
    uint32_t stats_valid, stats_bins, stats_row_begin, stats_width_px, stats_mode;
    float stats_view[16], stats_proj[16], stats_width, stats_height;
    uint32_t stats_count, stats_list_shift;
    // this draw
    float view[16], proj[16], width, height;
    uint32_t count, list_shift, bins_x, bin_row_begin, bin_row_end, block_cull, draw_mode, draw_serial, no_deep;
    // switches
    uint32_t deep_min, deep_factor, no_blend_order;
    float order_motion;
    uint32_t no_stat_shift, blend_order_stale, deep_row_major_on_motion, deep_units_last;
    uint32_t cu_count, occupancy;  // place_deep_units
    uint32_t list_current, visible;
    uint32_t measured_visible, measured_count, strip, no_block_list, block_test_always;   // block_test_mode
};
struct gs_draw_plan_debug_out {
    uint64_t entries, tiles16, room;
    uint32_t entries_valid, serial, overflow, deep_candidates, deep_share, view_valid, view_serial, visible;
    uint32_t blend_bins, order_ok, same_view;
    int32_t sx, sy;
    uint32_t order_wg, order_taken, deep_pass, deep_min, deep_factor;
    uint32_t unit_at, unit_wgs, list_shift;
    int32_t block_test;
};
extern "C" int gs_debug_draw_plan(const gs_draw_plan_debug_in* in, gs_draw_plan_debug_out* out);   // 0, or -1 on a NULL argument

// ... and for tests/test_bin_word.py: the word policy, and one splat position through both words of bin_word.hpp, packed and
// unpacked on the host by the functions the kernels use.  Rect coordinates are 16-px tiles, inclusive.
struct gs_bin_word_debug_in {
    uint32_t tiles_x, tiles_y, no_compact_bin_word;   // narrow_bin_word
    uint32_t visible, slot, x0, y0, x1, y1;           // the position: slot = its record's slot in the 256-splat block
};
struct gs_bin_word_debug_out {
    uint32_t narrow;                                   // 1: a draw of tiles_x x tiles_y tiles uses the 4-byte word
    uint32_t word;                                     // the 4-byte word ...
    uint32_t visible, escape, slot, x0, y0, x1, y1;    // ... unpacked (escape: the rect is not in the word, x0 .. y1 are 0)
    uint32_t wide_lo, wide_hi;                         // the 8-byte word ...
    uint32_t wide_visible, wide_slot, wide_x0, wide_y0, wide_x1, wide_y1;   // ... unpacked
};
extern "C" int gs_debug_bin_word(const gs_bin_word_debug_in* in, gs_bin_word_debug_out* out);   // 0, or -1 on a NULL argument

// ... and for tests/test_emit_units.py: k_bin_emit's live units of a draw whose slices hold cnt[0 .. slices) compacted splats.  The
// words are built as the kernel's prologue builds them (live_unit_word over the exclusive prefix of live_batches), and every unit
// l < min(total, room) is looked up with live_unit_find: (slice, batch, count) into units[3 * l ..].  Returns the draw's live units,
// or -1 on a NULL argument or slices == 0.
extern "C" int64_t gs_debug_live_units(const uint32_t* cnt, uint32_t slices, uint32_t* units, uint32_t room);
