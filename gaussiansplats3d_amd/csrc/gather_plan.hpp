// gather_plan.hpp — the HOST POLICY of an octree gather and its HAND-OVER to a sorter (gather_plan.cpp; host only: no device, no
// context; gs_tree and gs_sorter are names here, nothing more).
//
//   plan_gather   what one gs_tree_gather decides before it launches anything: the reference's two cull thresholds, the bucket
//                 scale of the plan kernels, whether the copy is deferred to the sorter, whether (and how far) the sorter's keep
//                 mask is zeroed, the leaf grid.  tree.hip fills a GatherPlanIn, calls plan_gather and acts on the plan.
//   hand-over     what a gather leaves a sorter is ONE record (GatherHandover) in one of three states, linked to the tree by one
//                 back-pointer (GatherTreeLink); the handover_* transitions below are the only code that writes either.
// Built with -ffp-contract=off: every fp64 product and sum rounds once, like the JS engine's - the thresholds decide, bit for bit,
// which leaves the kernel culls.  tests/test_gather_plan.py holds both halves to host models on a machine without a GPU
// (gs_debug_gather_plan, gs_debug_gather_handover).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsplat_hip.h"

// ---------------------------------------------------------------------------------------------------
// geometry the policy shares with the kernels (tree.hip, sorter.hip)
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t TREE_BUCKET_BITS = 18;
constexpr uint32_t TREE_BUCKETS = 1u << TREE_BUCKET_BITS;      // distance buckets of the gather's plan kernels
constexpr uint32_t PLAN_THREADS = 256;                          // leaves per workgroup of the per-leaf plan kernels
// bytes of a sorter's keep mask (a frustum-culled sort's key kernel writes whole 256-position windows, the gather zeroes a prefix)
inline size_t sorter_keep_mask_bytes(uint32_t max_count) { return (((size_t)max_count + 63) / 64 + 8) * 8; }

// ---------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------
struct GatherScene {
    double box[6];                 // sceneMin xyz, sceneMax xyz of the sub-tree
    double model_view[16];         // the modelView its leaves are tested under
    uint32_t empty, pad;           // the tree's filter kept nothing of the scene (no box)
};

struct GatherPlanIn {
    // the call (gs_gather_params)
    double model_view[16];         // the base modelView
    double fov_y_deg, render_width, render_height;
    uint32_t gather_all;
    // the tree
    uint32_t leaves, tree_splats;
    uint32_t scene_count;          // 1: a plain tree - scene[0] holds its box and the base modelView
    // the destination
    uint32_t has_sorter;           // the rest is 0 without one
    uint32_t sorter_flags;         // GS_SORT_*
    uint32_t frustum_cull;
    uint32_t max_count;            // its capacity (>= tree_splats, or gs_tree_gather refuses): sizes its keep mask, sorter_keep_mask_bytes
    uint32_t host_copy;            // the caller wants the list on the host as well
    uint32_t count_on_device;      // asynchronous gather: the count is not read back (no policy depends on it: the hand-over takes it)
    uint32_t no_defer;             // $GSPLAT_TREE_NO_DEFER, read by tree.hip at every gather (tests flip it inside one process)
    uint32_t pad;
    GatherScene scene[GS_MAX_SCENES];   // [scene_count]
};

struct GatherPlan {
    double thr_x, thr_y;           // cos(fovX/2) - 0.6, cos(fovY/2) - 0.6 (Viewer.js:1990-1996)
    double scale;                  // buckets per unit of distance
    uint32_t deferred;             // the plan stays in the tree: the sorter's next sort copies the lists (sorter.hip)
    uint32_t zero_keep, keep_words;   // k_tree_offsets zeroes this many 64-bit words of the sorter's keep mask
    uint32_t leaf_grid;            // workgroups of the per-leaf plan kernels (0: a tree without leaves launches nothing)
    uint32_t scene_table;          // several sub-trees: every leaf is tested under its own scene's modelView
    uint32_t pad;
};

// Total: any input yields a plan (scene_count is clamped to 1 .. GS_MAX_SCENES).
GatherPlan plan_gather(const GatherPlanIn& in);
// Matrix4.multiplyMatrices (three r160), its expression order, fp64, unfused: te = a x b, column-major
void gather_mat4_multiply(const double* a, const double* b, double* te);

// ---------------------------------------------------------------------------------------------------
// the hand-over
// ---------------------------------------------------------------------------------------------------
struct gs_sorter;
struct gs_tree;
struct GatherHandover;

enum : uint32_t {
    HANDOVER_NONE = 0,             // no gs_tree_gather has left this sorter a list
    HANDOVER_PLANNED = 1,          // the list is planned in the tree's tables (deferred): this sorter has still to copy it
    HANDOVER_COPIED = 2            // the list is in the sorter's idx_in
};

// The tree's side: who has still to copy its last planned gather.  Invariant: link.planner == &h exactly when
// h.state == HANDOVER_PLANNED and h.tree == &link.
struct GatherTreeLink {
    gs_tree* owner = nullptr;
    GatherHandover* planner = nullptr;
};

// The sorter's side.
struct GatherHandover {
    gs_sorter* owner = nullptr;
    uint32_t state = HANDOVER_NONE;
    GatherTreeLink* tree = nullptr;    // PLANNED: whose tables hold the list
    bool keep_zeroed = false;          // PLANNED: the gather zeroed this sorter's keep mask for a fused per-splat cull
    uint32_t count = 0;                // splatRenderCount of the list - an upper bound (the tree's splats) when ...
    bool count_on_device = false;      // ... the asynchronous gather left the real count in gs_sorter::gathered_dev
};

// A gather of `tree` (to the host: dst == nullptr) is about to overwrite the tree's tables.  A plan of dst's in ANOTHER tree is
// superseded.  Returns the sorter (never dst) that was still to copy this tree's previous plan: the caller copies that list into
// it NOW, on that sorter's own stream, before it launches anything - the record already says COPIED.
GatherHandover* handover_gather_begins(GatherTreeLink& tree, GatherHandover* dst);
// The gather is enqueued: dst (if any) holds a plan (deferred) or the list itself.  A tree without leaves hands over an empty
// list: deferred = false, count = 0, on the host.
void handover_gathered(GatherTreeLink& tree, GatherHandover* dst, bool deferred, bool keep_zeroed, uint32_t count, bool count_on_device);

// gs_sorter_sort_gathered: refused, or the counts of the sort
enum : uint32_t { HANDOVER_SORT_OK = 0, HANDOVER_SORT_NO_LIST = 1, HANDOVER_SORT_PARTIAL_ASYNC = 2 };
struct HandoverSort { uint32_t refused, sort_count, render_count, count_on_device; };
HandoverSort handover_sort_request(const GatherHandover& h, uint32_t sort_count);
// The sort copied the planned list into idx_in (SORT_GATHER_PLAIN: tree.hip's copy; SORT_GATHER_FUSED: its own key kernel).
void handover_copied(GatherHandover& h);

// A sort that does not consume the list may destroy what a gather left for a later gs_sorter_sort_gathered:
// ... a frustum-culled sort rewrites the keep mask the gather zeroed;
void handover_keep_mask_rewritten(GatherHandover& h);
// ... a host list or the compacting visibility front end overwrites idx_in.
void handover_list_overwritten(GatherHandover& h);

// The sorter is destroyed, or forgets everything that names splats by their numbering.
void handover_dropped(GatherHandover& h);
// The tree is destroyed: a sorter that was still to copy its plan has no list.
void handover_tree_destroyed(GatherTreeLink& tree);
// (A bound mesh that only reorders its storage changes nothing here: lists hold splat indexes.)

// ---------------------------------------------------------------------------------------------------
// Debug entries for the tests (pure host; typed by tests/gather_plan_cases.py, not in the public header).
// ---------------------------------------------------------------------------------------------------
extern "C" int gs_debug_gather_plan(const GatherPlanIn* in, GatherPlan* out);   // 0, or -1 on a NULL argument

// A script of events over two sorters (0, 1) and two trees (0, 1), starting from nothing; `sorter` 2 = no sorter (a host gather).
enum : uint32_t {
    HANDOVER_EV_GATHER = 0,        // tree, sorter | a: deferred  b: keep zeroed  c: count  d: count on device
    HANDOVER_EV_SORT_GATHERED,     // sorter | a: sort_count (an accepted sort copies a planned list)
    HANDOVER_EV_SORT_OTHER,        // sorter | a: host list  b: frustum cull  c: compacting visibility front end
    HANDOVER_EV_TREE_DESTROYED,    // tree (a new tree takes its number)
    HANDOVER_EV_SORTER_DESTROYED,  // sorter (a new sorter takes its number)
    HANDOVER_EV_FORGET_NUMBERING,  // sorter
    HANDOVER_EV_MESH_REORDERED,    // sorter
    HANDOVER_EV_KINDS
};
struct gs_handover_event { uint32_t kind, tree, sorter, a, b, c, d; };
struct gs_handover_step {
    uint32_t state[2], tree_of[2], keep_zeroed[2], count[2], count_on_device[2];   // per sorter; tree_of: 0, 1, or 2 = none
    uint32_t planner[2];           // per tree: 0, 1, or 2 = none
    uint32_t evicted;              // GATHER: the sorter that has to copy its planned list now (2 = none)
    uint32_t refused, sort_count, render_count, sort_on_device;   // SORT_GATHERED: HandoverSort
};
extern "C" int gs_debug_gather_handover(const gs_handover_event* events, uint32_t n, gs_handover_step* out);   // 0; -1: NULL or a bad event
