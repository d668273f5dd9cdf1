// draw_plan.cpp — see draw_plan.hpp.  Host arithmetic only; the comments that carry a measurement stand next to the rule it chose.
#include "draw_plan.hpp"

#include "bin_word.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

DrawFeedback read_feedback(const volatile uint32_t* mirror) {
    DrawFeedback f = {};
    if (!mirror) return f;
    f.view_serial = mirror[GS_MIRROR_VIEW_SERIAL];
    f.visible = mirror[GS_MIRROR_VISIBLE];
    const uint32_t t_lo = mirror[GS_MIRROR_TILES16_LO], t_hi = mirror[GS_MIRROR_TILES16_HI];
    f.tiles16 = ((uint64_t)t_hi << 32) | t_lo;
    f.view_valid = f.view_serial != 0u && mirror[GS_MIRROR_VIEW_SERIAL] == f.view_serial;   // nothing yet / a newer draw is writing
    f.serial = mirror[GS_MIRROR_SERIAL];
    f.overflow = mirror[GS_MIRROR_OVERFLOW] != 0u;
    const uint32_t e_lo = mirror[GS_MIRROR_ENTRIES_LO], e_hi = mirror[GS_MIRROR_ENTRIES_HI];
    f.entries = ((uint64_t)e_hi << 32) | e_lo;
    f.entries_valid = mirror[GS_MIRROR_SERIAL] == f.serial;                                  // a newer draw is writing
    f.deep_candidates = mirror[GS_MIRROR_DEEP_CANDIDATES];
    f.deep_share = mirror[GS_MIRROR_DEEP_SHARE];
    return f;
}

// Large lists only pay when splats are large enough to share them (a scene of tiny splats under 128-px lists makes every 32-px bin
// scan 16 bins' worth of entries: the capture-like C3S stand-in draws in 4.5 ms instead of 1.2).  Fed by gs_mesh_last_stats / a draw
// with statistics AND by the words every draw leaves in mapped host memory (mesh_read_view_share), so that a host that never asks
// for statistics - a viewer's render loop - gets the same bins a few frames later (profiles/r06w_motion_ab.txt: the flaw this closed).
// (with 8 % of hysteresis around each threshold: a camera that sits on one does not flip the size - and with it the entry
// statistics and the frame time - from draw to draw)
uint32_t adapt_list_shift(uint32_t current, uint64_t tiles16, uint32_t visible) {
    if (visible == 0u) return current;
    const float tiles = (float)tiles16, vis = (float)visible;
    static const uint32_t shifts[4] = {GS_LIST_SHIFT_SMALL, GS_LIST_SHIFT_LARGE, GS_LIST_SHIFT_BIG, GS_LIST_SHIFT_HUGE};
    static const float thr[3] = {GS_LIST_TILES_PER_SPLAT, GS_LIST_TILES_PER_SPLAT_BIG, GS_LIST_TILES_PER_SPLAT_HUGE};
    uint32_t level = 0;
    while (level < 3u && shifts[level] != current) level++;
    while (level < 3u && tiles >= 1.08f * thr[level] * vis) level++;
    while (level > 0u && tiles < 0.92f * thr[level - 1u] * vis) level--;
    return shifts[level];
}

// Where the block test runs, by the share of the splats that were in view at the mesh's last MEASURED full-frame draw (same box,
// tools/ab_libs.py, vertex stage): the separate k_block_test pays a launch (~5 us) to spare every dead block its workgroup's set-up,
// so it wins where most blocks are dead (C3, V/N 0.25: 58.0 -> 52.5 us; C2, 0.48: 35.0 against 35.9 inside the workgroups; any strip);
// a scene that is mostly in view keeps the test inside each workgroup (C3S, 0.65: 95.3 there vs 107.7 with no test at all); one
// that is all in view runs no test (C4, 0.998: 243.2 -> 219.2 us - the test's registers cost k_project a wave per SIMD).
// (profiles/r05z_ab_r03_vs_this_tree.txt, r05p_ab.txt)
int block_test_mode(uint32_t measured_visible, uint32_t measured_count, bool strip, bool block_cull, bool no_block_list, bool block_test_always) {
    const bool measured = measured_count > 0u;
    const bool all_live = measured && (uint64_t)measured_visible * 10u > (uint64_t)measured_count * 9u;
    const bool half_live = measured && !all_live && (uint64_t)measured_visible * 20u > (uint64_t)measured_count * 11u;
    // (strip: a strip of a scene that is mostly in view still drops most blocks)
    const bool test = block_cull && (!all_live || strip || block_test_always);
    const bool pretest = test && !no_block_list && (!half_live || strip || block_test_always);
    return pretest ? 1 : (test ? 0 : 2);
}

bool narrow_bin_word(uint32_t tiles_x, uint32_t tiles_y, const DrawSwitches& sw) {
    return tiles_x <= BIN_WORD_NARROW_TILES && tiles_y <= BIN_WORD_NARROW_TILES && !sw.no_compact_bin_word;
}

SchedulePlan plan_schedule(const ScheduleInputs& in) {
    const DrawSwitches& sw = in.sw;
    const PlanView& pp = in.now;
    SchedulePlan plan = {};
    const uint32_t blend_bins = in.bins_x * (in.bin_row_end - in.bin_row_begin);
    plan.blend_bins = blend_bins;
    // the previous draw's per-bin blend statistics order this draw's blend workgroups, if it drew the same bins
    // (only while the bins outnumber the resident workgroups by a small factor: an 8K frame's 32 k bins balance themselves by
    // backfilling, and ordering them in one workgroup would cost more than it gives)
    // deep pass: a bin qualifies when its previous draw walked >= deep_min (splat, quadrant) pairs and >= deep_factor x the mean bin
    // (4096 pairs.  C3S frame ms at 2048 / 3072 / 4096 / 6144 / 8192: 1.336 / 1.338 / 1.309 / 1.296 / 1.500 - k_deep_scan costs
    // 0.17 ms for 512 bins and is bound by its gathers, so: fewer, deeper bins; profiles/r03zz_kstats_C3S.txt)
    plan.deep_factor = sw.deep_factor;
    // (a GS_DRAW_ROP8 draw has no deep pass - rounding after every splat does not split into chunks - and must not raise its trigger)
    plan.deep_min = in.draw_mode == GS_DRAW_FP32 ? sw.deep_min : 0x7FFFFFFFu;
    const bool order_ok = blend_bins > 0 && blend_bins <= 8192u && in.stats.bins == blend_bins && in.stats.row_begin == in.bin_row_begin &&
                          in.stats.width_px == (uint32_t)pp.width && in.stats.draw_mode == in.draw_mode && !sw.no_blend_order;
    // (the same draw mode: a GS_DRAW_ROP8 draw walks its lists to the saturation depth twice or to their ends - its per-bin counters
    // say nothing about what an fp32 draw costs, and the other way round)
    plan.order_ok = order_ok;
    // ... and they ORDER this draw's blend workgroups only when that draw had THIS draw's view.  Heaviest-first from statistics of
    // the same view is worth 5-8 % of a frame (C3 demo pose 0.261 -> 0.248 ms, the orbit's poses held fixed 0.350 -> 0.322); from
    // a view 6 degrees away it is worth less than the workgroup that computes it costs - a moving camera draws its frames faster
    // in plain row-major order (C3 orbit 0.359 -> 0.349 ms per frame, C2 0.264 -> 0.255; profiles/r06g_orbit_gate.txt).  Two
    // stateless orders were built and measured as well, both no better than row-major: by the length of the list a bin scans (a
    // long list is a dense region that saturates at once: C2 fixed pose 0.327 vs 0.318 ms without any order, r06c) and a stride
    // permutation that makes the late starters a uniform sample of the screen (r06e: 0.3624 vs 0.3625).  The deep pass's
    // membership (which executor composites a bin, not when) keeps using the statistics of whatever view came before.
    const PlanView& lp = in.stats.view;
    const bool same_frame = in.stats.valid && memcmp(lp.proj, pp.proj, sizeof(pp.proj)) == 0 && lp.width == pp.width && lp.height == pp.height &&
                            lp.count == pp.count && lp.list_shift == pp.list_shift;
    bool same_view = same_frame && memcmp(lp.view, pp.view, sizeof(pp.view)) == 0;
    // ... or a view close to it.  Two things are taken from the two cameras (second half of round 6; tools/motion_ab.py):
    //  * how far the scene's centre of mass moved on screen, in whole bins: the schedule reads the statistics of the bin a bin's
    //    content came FROM (StatShift).  A camera turning about its own position shifts the whole picture - and the costly bins, and
    //    the deep pass's members - by that much: capture-like C3S turning 2 / 4 / 8 degrees per frame 2.14 / 2.77 / 3.78 -> 1.16 / 1.39 /
    //    2.06 ms per frame, C2 with the previous order at 4 / 8 degrees 0.3175 / 0.3139 -> 0.2913 / 0.3001 (row-major: 0.303)
    //    (profiles/r06zz_stat_shift_ab.txt; $GSPLAT_NO_STAT_SHIFT);
    //  * what that shift does NOT describe - parallax: how far points at half and at twice the centre's distance, on the previous
    //    camera's ray through the centre, end up from the centre in the new picture, in screen heights.  Orbiting the scene at 0.25 ...
    //    6 degrees per frame the previous frame's order beats row-major up to 2 degrees (C2 7-11 %, C3 1-2 % of the frame), is level
    //    at 3 and loses 2.5-3 % at 6 (profiles/r06w_motion_ab.txt): the order is taken below a parallax of 0.045 screen heights
    //    ($GSPLAT_ORDER_MOTION; 0 = the same view only).  Turning in place has none, at any speed.
    if (same_frame && !same_view && in.block_cull && in.centre_n > 0) {
        const float limit = sw.order_motion;
        const double inv_n = 1.0 / (double)in.centre_n;
        const float c[3] = {(float)(in.centre_sum[0] * inv_n), (float)(in.centre_sum[1] * inv_n), (float)(in.centre_sum[2] * inv_n)};
        auto window = [&](const PlanView& q, const float* p, float* xy) {       // (column-major matrices, window y up: project.hip)
            float v[4], o[4];
            for (int r = 0; r < 4; r++) v[r] = q.view[r] * p[0] + q.view[4 + r] * p[1] + q.view[8 + r] * p[2] + q.view[12 + r];
            for (int r = 0; r < 4; r++) o[r] = q.proj[r] * v[0] + q.proj[4 + r] * v[1] + q.proj[8 + r] * v[2] + q.proj[12 + r] * v[3];
            if (!(o[3] > 1e-6f)) return false;
            xy[0] = (o[0] / o[3] * 0.5f + 0.5f) * q.width;
            xy[1] = (o[1] / o[3] * 0.5f + 0.5f) * q.height;
            return true;
        };
        float was[2], is[2];
        if (window(lp, c, was) && window(pp, c, is)) {
            const float dx = (is[0] - was[0]) / (float)GS_BIN, dy = (is[1] - was[1]) / (float)GS_BIN;
            const bool shift_ok = fabsf(dx) < 4096.0f && fabsf(dy) < 4096.0f && !sw.no_stat_shift;   // (false for NaN)
            if (shift_ok) {
                plan.sx = (int32_t)lrintf(dx);
                plan.sy = (int32_t)lrintf(dy);
            }
            // the previous camera's position in the splats' own space: -A^-1 b of its modelView = [A | b]
            const float* V = lp.view;
            const float a00 = V[0], a10 = V[1], a20 = V[2], a01 = V[4], a11 = V[5], a21 = V[6], a02 = V[8], a12 = V[9], a22 = V[10];
            const float c00 = a11 * a22 - a12 * a21, c01 = a02 * a21 - a01 * a22, c02 = a01 * a12 - a02 * a11;
            const float det = a00 * c00 + a10 * c01 + a20 * c02;
            const float b0 = V[12], b1 = V[13], b2 = V[14], id = 1.0f / det;
            const float eye[3] = {-(c00 * b0 + c01 * b1 + c02 * b2) * id,
                                  -((a12 * a20 - a10 * a22) * b0 + (a00 * a22 - a02 * a20) * b1 + (a02 * a10 - a00 * a12) * b2) * id,
                                  -((a10 * a21 - a11 * a20) * b0 + (a01 * a20 - a00 * a21) * b1 + (a00 * a11 - a01 * a10) * b2) * id};
            float parallax = 0.0f;
            bool seen = fabsf(det) > 1e-20f;
            for (int k = 0; k < 2 && seen; k++) {
                const float t = k ? 2.0f : 0.5f;
                const float p[3] = {eye[0] + t * (c[0] - eye[0]), eye[1] + t * (c[1] - eye[1]), eye[2] + t * (c[2] - eye[2])};
                float at[2];
                seen = window(pp, p, at);
                if (seen) parallax = fmaxf(parallax, sqrtf((at[0] - is[0]) * (at[0] - is[0]) + (at[1] - is[1]) * (at[1] - is[1])));
            }
            // (without the shift the whole motion counts, not only the parallax)
            const float moved = (parallax + (shift_ok ? 0.0f : sqrtf(dx * dx + dy * dy) * (float)GS_BIN)) / fmaxf(pp.height, 1.0f);
            same_view = seen && moved <= limit;            // (NaN compares false)
        }
    }
    plan.same_view = same_view;
    const bool stale_order = sw.blend_order_stale;   // (A/B: rounds 2-5 - order from whatever draw came before)
    // The deep pass runs when the last draw whose verdict has arrived (mapped host word, no synchronisation) left bins over the
    // threshold - the decision only moves work between executors, the pixels do not depend on it (tile_blend.hip)
    plan.deep_pass = order_ok && in.draw_mode == GS_DRAW_FP32 && !in.no_deep && in.feedback.deep_candidates > 0u;
    // (+ one workgroup that orders the blend's bins and names the deep pass's members)
    // (that workgroup also raises the deep pass's trigger, so under a camera that keeps moving it still runs when the pass is on,
    // for scenes of tiny splats - the ones that grow deep bins - and every 8th draw otherwise)
    plan.order_wg = order_ok && (same_view || stale_order || plan.deep_pass || pp.list_shift == GS_LIST_SHIFT_SMALL || (in.draw_serial & 7u) == 7u);
    // ... and whenever the deep pass runs: its frames have the long tail that an order - even one from a view several degrees away -
    // and the pass's workgroups behind the costliest bins (tile_blend.hip) shorten.  Capture-like C3S, orbit at 3 / 6 / 12 degrees per
    // frame: 1.24 / 1.356 / 1.54 -> 1.18 / 1.31 / 1.51 ms, turning 4 degrees per frame 2.84 -> 2.77, never slower
    // (profiles/r06zz_deep_keeps_order_ab.txt; $GSPLAT_DEEP_ROW_MAJOR_ON_MOTION=1 is the earlier rule).
    plan.order_taken = order_ok && (same_view || stale_order || (plan.deep_pass && !sw.deep_row_major_on_motion));
    return plan;
}

// two per CU - or, when the pass's bins were most of the previous draw's walk, 0.6 of their share of the resident workgroups
// (C3S: share 0.55, best at a third of the workgroups whatever AT is: 256 / 512 / 768 / 1536 -> 1.30 / 1.125 / 1.15 / 1.20 ms;
// with exactly the share, 1.17)
constexpr float DEEP_WGS_PER_SHARE = 0.6f;

// Their waves take (bin, quadrant, chunk) units from a list until it is empty, so any number of them finishes the pass; what
// matters is WHEN they run against the per-bin workgroups (capture-like C3S, profiles/r06z_deep_unit_ab.txt):
//  * bins in costliest-first order (this view's statistics): the units used to come last, started 340 us into a 985 us launch and
//    ended it alone; all 1536 of them in front (AT = 0) crowd the costliest bins out.  Two workgroups per CU behind the deep bins'
//    own (empty) workgroups and the ~1.5 costliest bins per CU: frame 1.300 -> 1.13 ms at the demo pose, 1.300 -> 1.105 in the mean
//    of the orbit's poses held fixed;
//  * bins in row-major order (the camera moved on: no order): units are the fine-grained work that fills the end of the launch -
//    in the middle they cost 13 % (moving camera 1.35 -> 1.52 ms) - so they stay last, all of them.
DeepUnits place_deep_units(const SchedulePlan& plan, uint32_t bins, uint32_t cu_count, uint32_t occupancy, const DrawFeedback& feedback,
                           const DrawSwitches& sw) {
    DeepUnits du;
    // (as many workgroups as the device holds at `occupancy` per CU: their waves loop over the unit list)
    du.unit_wgs = plan.deep_pass ? cu_count * occupancy : 0u;
    du.unit_at = bins;
    if (plan.deep_pass && plan.order_taken && !sw.deep_units_last) {
        const uint32_t cus = cu_count;
        const uint32_t deep_hint = feedback.deep_candidates;                     // bins the last verdict put in the pass
        const float share = (float)std::min(feedback.deep_share, 1024u) * (1.0f / 1024.0f);
        const float k = DEEP_WGS_PER_SHARE;
        du.unit_wgs = std::min(du.unit_wgs, std::max(2u * cus, (uint32_t)(k * share * (float)du.unit_wgs + 0.5f)));
        du.unit_at = std::min(bins, std::min(deep_hint, (uint32_t)GS_DEEP_MAX_BINS) + cus + cus / 2u);
    }
    return du;
}

static PlanView plan_view(const float* view, const float* proj, float width, float height, uint32_t count, uint32_t list_shift) {
    PlanView v;
    memcpy(v.view, view, sizeof(v.view));
    memcpy(v.proj, proj, sizeof(v.proj));
    v.width = width; v.height = height; v.count = count; v.list_shift = list_shift;
    return v;
}

extern "C" int gs_debug_draw_plan(const gs_draw_plan_debug_in* in, gs_draw_plan_debug_out* out) {
    if (!in || !out) return -1;
    const DrawFeedback fb = read_feedback(in->mirror);
    ScheduleInputs si = {};
    si.stats.valid = in->stats_valid != 0u;
    si.stats.bins = in->stats_bins; si.stats.row_begin = in->stats_row_begin; si.stats.width_px = in->stats_width_px; si.stats.draw_mode = in->stats_mode;
    si.stats.view = plan_view(in->stats_view, in->stats_proj, in->stats_width, in->stats_height, in->stats_count, in->stats_list_shift);
    si.now = plan_view(in->view, in->proj, in->width, in->height, in->count, in->list_shift);
    si.bins_x = in->bins_x; si.bin_row_begin = in->bin_row_begin; si.bin_row_end = in->bin_row_end;
    si.block_cull = in->block_cull; si.draw_mode = in->draw_mode; si.draw_serial = in->draw_serial; si.no_deep = in->no_deep != 0u;
    memcpy(si.centre_sum, in->centre_sum, sizeof(si.centre_sum));
    si.centre_n = in->centre_n;
    si.feedback = fb;
    si.sw.deep_min = in->deep_min; si.sw.deep_factor = in->deep_factor; si.sw.no_blend_order = in->no_blend_order != 0u;
    si.sw.order_motion = in->order_motion; si.sw.no_stat_shift = in->no_stat_shift != 0u; si.sw.blend_order_stale = in->blend_order_stale != 0u;
    si.sw.deep_row_major_on_motion = in->deep_row_major_on_motion != 0u; si.sw.deep_units_last = in->deep_units_last != 0u;
    const SchedulePlan plan = plan_schedule(si);
    const DeepUnits du = place_deep_units(plan, plan.blend_bins, in->cu_count, in->occupancy, fb, si.sw);
    *out = gs_draw_plan_debug_out();
    out->entries = fb.entries; out->tiles16 = fb.tiles16; out->room = entry_room(in->need);
    out->entries_valid = fb.entries_valid; out->serial = fb.serial; out->overflow = fb.overflow;
    out->deep_candidates = fb.deep_candidates; out->deep_share = fb.deep_share;
    out->view_valid = fb.view_valid; out->view_serial = fb.view_serial; out->visible = fb.visible;
    out->blend_bins = plan.blend_bins; out->order_ok = plan.order_ok; out->same_view = plan.same_view;
    out->sx = plan.sx; out->sy = plan.sy;
    out->order_wg = plan.order_wg; out->order_taken = plan.order_taken; out->deep_pass = plan.deep_pass;
    out->deep_min = plan.deep_min; out->deep_factor = plan.deep_factor;
    out->unit_at = du.unit_at; out->unit_wgs = du.unit_wgs;
    out->list_shift = adapt_list_shift(in->list_current, in->tiles16, in->visible);
    out->block_test = block_test_mode(in->measured_visible, in->measured_count, in->strip != 0u, in->block_cull != 0u, in->no_block_list != 0u,
                                      in->block_test_always != 0u);
    return 0;
}

extern "C" int gs_debug_bin_word(const gs_bin_word_debug_in* in, gs_bin_word_debug_out* out) {
    if (!in || !out) return -1;
    DrawSwitches sw = {};
    sw.no_compact_bin_word = in->no_compact_bin_word != 0u;
    *out = gs_bin_word_debug_out();
    out->narrow = narrow_bin_word(in->tiles_x, in->tiles_y, sw) ? 1u : 0u;
    const BinRect r = {in->x0 | (in->y0 << 16), in->x1 | (in->y1 << 16)};
    out->word = bin_word_pack_narrow(in->visible != 0u, in->slot, r);
    const BinWordOut n = bin_word_unpack_narrow(out->word);
    out->visible = n.visible; out->escape = n.escape; out->slot = n.slot;
    if (n.visible && !n.escape) { out->x0 = n.rect.lo & 0xFFFFu; out->y0 = n.rect.lo >> 16; out->x1 = n.rect.hi & 0xFFFFu; out->y1 = n.rect.hi >> 16; }
    const BinWordWide w = bin_word_pack_wide(in->visible != 0u, in->slot, r);
    out->wide_lo = w.x; out->wide_hi = w.y;
    const BinWordOut u = bin_word_unpack_wide(w);
    out->wide_visible = u.visible; out->wide_slot = u.slot;
    out->wide_x0 = u.rect.lo & 0xFFFFu; out->wide_y0 = u.rect.lo >> 16; out->wide_x1 = u.rect.hi & 0xFFFFu; out->wide_y1 = u.rect.hi >> 16;
    return 0;
}

extern "C" int64_t gs_debug_live_units(const uint32_t* cnt, uint32_t slices, uint32_t* units, uint32_t room) {
    if (!cnt || slices == 0u || (!units && room != 0u)) return -1;
    std::vector<uint32_t> words(slices);
    uint32_t total = 0;
    for (uint32_t b = 0; b < slices; b++) {
        words[b] = live_unit_word(total, cnt[b]);
        total += live_batches(cnt[b]);
    }
    for (uint32_t l = 0; l < std::min(total, room); l++) {
        const LiveUnit u = live_unit_find([&](uint32_t b) { return words[b]; }, slices, total, l);
        units[3u * l] = u.slice; units[3u * l + 1u] = u.batch; units[3u * l + 2u] = u.count;
    }
    return (int64_t)total;
}
