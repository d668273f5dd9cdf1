// gather_plan.cpp — the host policy of an octree gather and its hand-over to a sorter (gather_plan.hpp).
#include "gather_plan.hpp"

#include <math.h>

void gather_mat4_multiply(const double* a, const double* b, double* te) {
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            te[r + 4 * c] = a[r] * b[4 * c] + a[r + 4] * b[4 * c + 1] + a[r + 8] * b[4 * c + 2] + a[r + 12] * b[4 * c + 3];
}

GatherPlan plan_gather(const GatherPlanIn& in) {
    GatherPlan pl = {};
    const uint32_t scenes = in.scene_count < 1u ? 1u : in.scene_count > GS_MAX_SCENES ? GS_MAX_SCENES : in.scene_count;
    pl.scene_table = scenes > 1u;
    // Viewer.js:1990-1996
    const double deg2rad = 3.14159265358979323846 / 180.0;              // THREE.MathUtils.DEG2RAD = Math.PI / 180
    const double focal = (in.render_height / 2.0) / tan(in.fov_y_deg / 2.0 * deg2rad);
    const double fov_x2 = atan(in.render_width / 2.0 / focal), fov_y2 = atan(in.render_height / 2.0 / focal);
    pl.thr_x = cos(fov_x2) - .6;
    pl.thr_y = cos(fov_y2) - .6;
    // bucket scale: the farthest a leaf centre can be from the eye = the farthest corner of the scene box under this modelView
    // (the distance is convex in the point); the order never depends on it (tree_bucket clamps), only how the leaves spread.
    // Several sub-trees: the largest over the scenes, each scene's box under its own modelView.
    double far = 0.0;
    for (uint32_t sc = 0; sc < 8u * scenes; sc++) {
        const uint32_t c = sc & 7u;
        const GatherScene& s = in.scene[sc >> 3];
        if (s.empty) continue;
        const double *mn = s.box, *mx = s.box + 3, *e = s.model_view;
        const double x = (c & 1) ? mx[0] : mn[0], y = (c & 2) ? mx[1] : mn[1], z = (c & 4) ? mx[2] : mn[2];
        double w = e[3] * x + e[7] * y + e[11] * z + e[15];
        w = w != 0.0 ? 1.0 / w : 1.0;
        const double vx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w, vy = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w,
                     vz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w;
        const double d = sqrt(vx * vx + vy * vy + vz * vz);
        if (d > far) far = d;
    }
    pl.scale = (far > 0.0 && far < 1e300) ? (double)TREE_BUCKETS / (far * 1.0001) : 1.0;
    // The copy is DEFERRED to the sorter when nothing but the sorter will read the list: a full sort of a static scene then
    // copies the lists, keys them (and tests them against the frustum) in one kernel that streams the centres in leaf order
    // (sorter.hip, k_tree_copy_keys); any other sort copies first (gs_tree_copy_plain) and goes on as before.
    // (never for a tree of several sub-trees: the fused copy and its leaf-ordered centre planes know one modelView)
    pl.deferred = in.leaves && in.has_sorter && !in.host_copy && !(in.sorter_flags & GS_SORT_DYNAMIC) && !in.no_defer && !pl.scene_table;
    pl.zero_keep = pl.deferred && in.frustum_cull;          // the fused copy ORs its keep bits into a zeroed mask
    pl.keep_words = pl.zero_keep ? (uint32_t)(((size_t)in.tree_splats + 63) / 64 + 2) : 0u;
    pl.leaf_grid = (uint32_t)(((uint64_t)in.leaves + PLAN_THREADS - 1u) / PLAN_THREADS);
    return pl;
}

extern "C" int gs_debug_gather_plan(const GatherPlanIn* in, GatherPlan* out) {
    if (!in || !out) return -1;
    *out = plan_gather(*in);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// the hand-over
// ---------------------------------------------------------------------------------------------------
// h's plan (if it holds one) is no longer wanted: both ends of the link go
static void unlink(GatherHandover& h) {
    if (h.state == HANDOVER_PLANNED) h.tree->planner = nullptr;
    h.tree = nullptr;
    h.keep_zeroed = false;
}

GatherHandover* handover_gather_begins(GatherTreeLink& tree, GatherHandover* dst) {
    if (dst && dst->state == HANDOVER_PLANNED && dst->tree != &tree) handover_copied(*dst);   // superseded: idx_in is about to be rewritten
    GatherHandover* evicted = tree.planner != dst ? tree.planner : nullptr;
    if (evicted) handover_copied(*evicted);
    return evicted;
}

void handover_gathered(GatherTreeLink& tree, GatherHandover* dst, bool deferred, bool keep_zeroed, uint32_t count, bool count_on_device) {
    if (!dst) return;
    unlink(*dst);
    dst->state = deferred ? HANDOVER_PLANNED : HANDOVER_COPIED;
    if (deferred) {
        dst->tree = &tree;
        dst->keep_zeroed = keep_zeroed;
        tree.planner = dst;
    }
    dst->count = count;
    dst->count_on_device = count_on_device;
}

HandoverSort handover_sort_request(const GatherHandover& h, uint32_t sort_count) {
    if (h.state == HANDOVER_NONE) return {HANDOVER_SORT_NO_LIST, 0u, 0u, 0u};
    if (h.count_on_device)                                     // h.count = the tree's splat count, an upper bound
        return {sort_count >= h.count ? HANDOVER_SORT_OK : HANDOVER_SORT_PARTIAL_ASYNC, h.count, h.count, 1u};
    return {HANDOVER_SORT_OK, sort_count > h.count ? h.count : sort_count, h.count, 0u};   // Math.min(queuedSorts.shift(), splatRenderCount)
}

void handover_copied(GatherHandover& h) {
    if (h.state != HANDOVER_PLANNED) return;
    unlink(h);
    h.state = HANDOVER_COPIED;
}

// A planned gather's fused copy ORs its keep bits into a mask the GATHER zeroed - a frustum-culled sort between the gather and
// its sort rewrites that mask, so the copy falls back to the plain one + the ordinary key kernel (sort_plan.cpp reads keep_zeroed).
void handover_keep_mask_rewritten(GatherHandover& h) { h.keep_zeroed = false; }

// A list that was already copied into idx_in is gone once a host list or k_mask_compact overwrites it.  A PLANNED list still
// lives in the tree's tables and stays - and so does a COPIED one under the STREAMING visibility front end, which writes pay_in
// and leaves idx_in alone: that front end does not call this.
void handover_list_overwritten(GatherHandover& h) {
    if (h.state == HANDOVER_COPIED) h.state = HANDOVER_NONE, h.count = 0, h.count_on_device = false;
}

void handover_dropped(GatherHandover& h) {
    unlink(h);
    h.state = HANDOVER_NONE;
    h.count = 0;
    h.count_on_device = false;
}

void handover_tree_destroyed(GatherTreeLink& tree) {
    if (tree.planner) handover_dropped(*tree.planner);
}

extern "C" int gs_debug_gather_handover(const gs_handover_event* events, uint32_t n, gs_handover_step* out) {
    if (!events || !out) return -1;
    GatherHandover sorter[2];
    GatherTreeLink tree[2];
    for (uint32_t k = 0; k < n; k++) {
        const gs_handover_event& ev = events[k];
        gs_handover_step& o = out[k];
        o = gs_handover_step();
        o.evicted = 2u;
        if (ev.kind >= HANDOVER_EV_KINDS || ev.tree > 1u || ev.sorter > (ev.kind == HANDOVER_EV_GATHER ? 2u : 1u)) return -1;
        GatherHandover* s = ev.sorter < 2u ? &sorter[ev.sorter] : nullptr;
        switch (ev.kind) {
        case HANDOVER_EV_GATHER: {
            const GatherHandover* evicted = handover_gather_begins(tree[ev.tree], s);
            if (evicted) o.evicted = (uint32_t)(evicted - sorter);
            handover_gathered(tree[ev.tree], s, ev.a != 0u, ev.b != 0u, ev.c, ev.d != 0u);
            break;
        }
        case HANDOVER_EV_SORT_GATHERED: {
            const HandoverSort r = handover_sort_request(*s, ev.a);
            o.refused = r.refused; o.sort_count = r.sort_count; o.render_count = r.render_count; o.sort_on_device = r.count_on_device;
            if (!r.refused) handover_copied(*s);
            break;
        }
        case HANDOVER_EV_SORT_OTHER:
            if (ev.b) handover_keep_mask_rewritten(*s);
            if (ev.a || ev.c) handover_list_overwritten(*s);
            break;
        case HANDOVER_EV_TREE_DESTROYED: handover_tree_destroyed(tree[ev.tree]); break;
        case HANDOVER_EV_SORTER_DESTROYED:
        case HANDOVER_EV_FORGET_NUMBERING: handover_dropped(*s); break;
        default: break;                                        // the mesh reordered: nothing
        }
        for (uint32_t i = 0; i < 2u; i++) {
            o.state[i] = sorter[i].state;
            o.tree_of[i] = sorter[i].tree ? (uint32_t)(sorter[i].tree - tree) : 2u;
            o.keep_zeroed[i] = sorter[i].keep_zeroed;
            o.count[i] = sorter[i].count;
            o.count_on_device[i] = sorter[i].count_on_device;
            o.planner[i] = tree[i].planner ? (uint32_t)(tree[i].planner - sorter) : 2u;
        }
    }
    return 0;
}
