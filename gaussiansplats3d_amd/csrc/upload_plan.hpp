// upload_plan.hpp — the host policy of an upload into a mesh (mesh.hip, bounds.hip): which splats own storage slots, where one
// upload is cut into fresh and non-fresh segments, which storage blocks get new boxes, and where a segment's arrays sit in the
// staging buffer.  Host only: no HIP, no gs_mesh, no context.  tests/test_upload_plan.py holds it to a bitmap model through
// gs_debug_upload_plan; tests/tools/upload_plan_fuzz.cpp is the stand-alone program for a sanitizer run.  Also here: the plans of
// gs_mesh_remove / gs_sorter_remove (plan_remove) and of gs_mesh_reorder (plan_reorder), each with its debug entry, test and program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

constexpr uint32_t UPLOAD_MAX_SPLATS = 1u << 28;           // gs_mesh_create's limit: spans of a plan end at or below it
constexpr uint32_t UPLOAD_BLOCK = 256;                     // splats per storage block (gs_mesh::block_box)

struct SlotRange { uint32_t begin, end; };                 // [begin, end)
struct SlotCut { uint32_t begin, end; bool fresh; };       // fresh: none of its splats owns a slot; else all of them do

// The splats that own storage slots (an upload has seen them): ranges that are non-empty, sorted by begin, disjoint and never
// adjacent - ranges that touch are one range.  A fresh segment is stored in its own slots, so the splats of a range occupy
// exactly the storage positions of that range.
class SlottedRanges {
public:
    // the one range that contains [from, from + count) whole (summed in 64 bits), or nullptr
    const SlotRange* holding(uint32_t from, uint32_t count) const;
    // [from, end) as consecutive segments, cut at the ranges' borders
    std::vector<SlotCut> cut(uint32_t from, uint32_t end) const;
    // merges [from, end) in
    void add(uint32_t from, uint32_t end);
    const std::vector<SlotRange>& ranges() const { return r_; }
private:
    std::vector<SlotRange> r_;
};

// One segment of an upload: splats [begin, end), and the storage blocks [b0, b1) whose boxes it invalidates.  A fresh segment
// receives the slots [begin, end).  Splats uploaded before keep THEIR slots, scattered over the Morton run(s) of the earlier
// upload(s) - anywhere inside the range that held the segment before this upload: all of that range's blocks are redone.
// (only the segment's own span was redone, so a block kept the box of the data it held before the edit and k_project's
// block cull could drop splats that had moved into view.)
struct UploadSegment {
    uint32_t begin, end;
    bool fresh;                    // the cut's verdict; always true on a mesh that keeps upload order
    uint32_t b0, b1;
};
// the segments of an upload of [from, from + count), from + count <= UPLOAD_MAX_SPLATS, in order; `ranges` as they are BEFORE it
std::vector<UploadSegment> plan_upload(const SlottedRanges& ranges, uint32_t from, uint32_t count, bool reorder);

// Where a segment's arrays sit in the staging buffer: centres float [3n] at 0 | covariance float [6n] or half bits [6n] | SH half
// bits or uint8 [ncoef n] | rgba uint8 [4n]; every plane starts on a multiple of 256 bytes.  The decode kernels of
// asset_decode.hip write the same planes.
struct UploadLayout {
    uint32_t ncoef;                // SH values per splat the source stages (0: none)
    bool sh_u8;                    // ... as uint8 (a GS_MESH_SH_U8 mesh whose source stages them), else half bits
    size_t off_cov, off_sh, off_rgba;
    size_t bytes;                  // the staging buffer holds at least this much
};
// source_stages_sh_u8: the source stages the uint8 SH of a GS_MESH_SH_U8 mesh too (the host path hands those to
// gs_mesh_upload_sh_u8 instead)
UploadLayout upload_layout(uint32_t count, bool cov_half, bool mesh_sh_u8, uint32_t sh_degree, bool source_stages_sh_u8);

// ---------------------------------------------------------------------------------------------------
// Removing splats from a mesh or a sorter (mesh_edit.hip, sorter.hip: gs_mesh_remove / gs_sorter_remove).  The removed ranges go
// away, every survivor i becomes i - (removed positions below i), and - because a fresh segment occupies the storage slots of its
// own index range - the storage spans move by the same shift as the indexes.  That holds only while no border of a removed range
// falls inside a Morton run (the span of one fresh segment of a mesh that re-orders: its splats are scattered over the whole run),
// so the mesh remembers its runs - SlottedRanges merges the ones that touch - and plan_remove refuses such a border.
constexpr uint32_t REMOVE_MAX_RANGES = 32;                 // GS_MAX_SCENES
struct RemoveMove { uint32_t begin, end, shift; };         // the survivors [begin, end) (old numbering) move down by shift > 0
struct RemovePlan {
    const char* refused = nullptr;                         // why not (then nothing else is filled in), or nullptr
    std::vector<SlotRange> cuts;                           // the removed ranges clipped to [0, uploaded), none empty, ascending
    std::vector<RemoveMove> moves;                         // ascending; together with the untouched head they are the survivors
    std::vector<SlotRange> runs;                           // the runs that survive, shifted (never merged)
    SlottedRanges slotted;                                 // the slotted ranges that survive, shifted (those that now touch are one)
    uint32_t removed = 0;                                  // positions below `uploaded` that go away
    uint32_t uploaded = 0;                                 // the uploaded count afterwards
    uint32_t first_block = 0;                              // first storage block whose content changes (removed > 0)
};
// ranges: n pairs {from, count} in the caller's numbering - 1 <= n <= REMOVE_MAX_RANGES, ascending, disjoint, non-empty, inside
// [0, max_count].  runs: sorted, disjoint, inside [0, uploaded) (empty for a sorter and a mesh that keeps upload order).
RemovePlan plan_remove(const std::vector<SlotRange>& runs, const SlottedRanges& slotted, uint32_t uploaded, uint32_t max_count,
                       bool reorder, const uint32_t* ranges, uint32_t n);

// ---------------------------------------------------------------------------------------------------
// Folding the Morton runs of [from, from + count) into one (mesh_edit.hip: gs_mesh_reorder).  The runs in the range keep its
// storage slots between them, so the range must be their union: all of it uploaded, neither border inside a run.  The checks, in
// this order: count == 0 does nothing; a range beyond `uploaded` is refused (on any mesh); a mesh that keeps upload order does
// nothing; a never-uploaded position and a border inside a run are refused; a range of at most one run does nothing.
struct ReorderPlan {
    const char* refused = nullptr;                         // why not (then nothing else is filled in), or nullptr
    bool noop = false;                                     // nothing to do (then nothing else is filled in)
    std::vector<SlotRange> runs;                           // the runs afterwards: those of the range are the one run [from, from + count)
    uint32_t first_block = 0, end_block = 0;               // the storage blocks [first_block, end_block) get new boxes
};
ReorderPlan plan_reorder(const std::vector<SlotRange>& runs, const SlottedRanges& slotted, uint32_t uploaded, bool reorder, uint32_t from,
                         uint32_t count);

// ---------------------------------------------------------------------------------------------------
// Debug entry for the tests (pure host; typed by tests/upload_plan_cases.py, not in the public header).  Flags are uint32 (0 / 1).
constexpr uint32_t UPLOAD_DEBUG_MAX = 64;                  // ranges in, ranges out, segments
struct gs_upload_plan_debug_in {
    uint32_t n_ranges;                                     // the state before the upload: add()ed in this order
    uint32_t ranges[UPLOAD_DEBUG_MAX][2];
    uint32_t from, count, reorder;                         // the upload
    uint32_t hold_from, hold_count;                        // holding(), asked before the upload
    uint32_t layout_count, cov_half, mesh_sh_u8, sh_degree, source_stages_sh_u8;
};
struct gs_upload_plan_debug_out {
    uint32_t n_segments;
    uint32_t segments[UPLOAD_DEBUG_MAX][5];                // begin, end, fresh, b0, b1
    uint32_t n_before;                                     // the ranges the inputs made
    uint32_t before[UPLOAD_DEBUG_MAX][2];
    uint32_t n_after;                                      // ... and after add(from, from + count)
    uint32_t after[UPLOAD_DEBUG_MAX][2];
    uint32_t held, hold_begin, hold_end;
    uint32_t ncoef, sh_u8;
    uint64_t off_cov, off_sh, off_rgba, bytes;
};
// 0; -1 on a NULL argument, an empty or reversed input range, a span beyond UPLOAD_MAX_SPLATS or more than UPLOAD_DEBUG_MAX rows
extern "C" int gs_debug_upload_plan(const gs_upload_plan_debug_in* in, gs_upload_plan_debug_out* out);

// ... and for plan_remove (typed by tests/remove_plan_cases.py)
struct gs_remove_plan_debug_in {
    uint32_t n_runs;                                       // the state before: the runs as the mesh remembers them
    uint32_t runs[UPLOAD_DEBUG_MAX][2];
    uint32_t n_slotted;                                    // ... and its slotted ranges, add()ed in this order
    uint32_t slotted[UPLOAD_DEBUG_MAX][2];
    uint32_t uploaded, max_count, reorder;
    uint32_t n_ranges;                                     // the call: {from, count} pairs, handed on as they are
    uint32_t ranges[UPLOAD_DEBUG_MAX][2];
};
struct gs_remove_plan_debug_out {
    uint32_t refused;                                      // 1: the plan refused the call (nothing else is filled in)
    uint32_t n_moves;
    uint32_t moves[UPLOAD_DEBUG_MAX][3];                   // begin, end, shift
    uint32_t n_runs;
    uint32_t runs[UPLOAD_DEBUG_MAX][2];
    uint32_t n_slotted;
    uint32_t slotted[UPLOAD_DEBUG_MAX][2];
    uint32_t removed, uploaded, first_block;
};
// 0; -1 on a NULL argument, more than UPLOAD_DEBUG_MAX rows, or a state no mesh can be in (runs or slotted ranges that are empty,
// unsorted, overlapping or beyond `uploaded`; uploaded > max_count; max_count > UPLOAD_MAX_SPLATS)
extern "C" int gs_debug_remove_plan(const gs_remove_plan_debug_in* in, gs_remove_plan_debug_out* out);

// ... and for plan_reorder (typed by tests/reorder_plan_cases.py)
struct gs_reorder_plan_debug_in {
    uint32_t n_runs;                                       // the state before: the runs as the mesh remembers them
    uint32_t runs[UPLOAD_DEBUG_MAX][2];
    uint32_t n_slotted;                                    // ... and its slotted ranges, add()ed in this order
    uint32_t slotted[UPLOAD_DEBUG_MAX][2];
    uint32_t uploaded, reorder;
    uint32_t from, count;                                  // the call
};
struct gs_reorder_plan_debug_out {
    uint32_t refused;                                      // 1: the plan refused the call (nothing else is filled in)
    uint32_t noop;                                         // 1: nothing to do (nothing else is filled in)
    uint32_t n_runs;
    uint32_t runs[UPLOAD_DEBUG_MAX][2];
    uint32_t first_block, end_block;
};
// 0; -1 on a NULL argument, more than UPLOAD_DEBUG_MAX rows, or a state no mesh can be in (as gs_debug_remove_plan; uploaded >
// UPLOAD_MAX_SPLATS)
extern "C" int gs_debug_reorder_plan(const gs_reorder_plan_debug_in* in, gs_reorder_plan_debug_out* out);
