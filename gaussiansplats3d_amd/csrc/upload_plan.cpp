// upload_plan.cpp — see upload_plan.hpp.  Host only.
#include "upload_plan.hpp"

#include <algorithm>

const SlotRange* SlottedRanges::holding(uint32_t from, uint32_t count) const {
    for (const SlotRange& r : r_)
        if (r.begin <= from && (uint64_t)from + count <= r.end) return &r;   // ranges that touch are merged, so one must cover it
    return nullptr;
}

std::vector<SlotCut> SlottedRanges::cut(uint32_t from, uint32_t end) const {
    std::vector<SlotCut> cuts;
    uint32_t pos = from;
    for (const SlotRange& r : r_) {
        if (pos >= end || r.begin >= end) break;
        if (r.end <= pos) continue;
        if (r.begin > pos) { cuts.push_back({pos, r.begin, true}); pos = r.begin; }
        const uint32_t stop = std::min(r.end, end);
        cuts.push_back({pos, stop, false});
        pos = stop;
    }
    if (pos < end) cuts.push_back({pos, end, true});
    return cuts;
}

void SlottedRanges::add(uint32_t from, uint32_t end) {
    if (from >= end) return;
    std::vector<SlotRange> merged;
    SlotRange cur = {from, end};
    bool placed = false;
    for (const SlotRange& r : r_) {
        if (r.end < cur.begin) merged.push_back(r);
        else if (r.begin > cur.end) {                      // (sorted: so is every range after it - cur is final)
            if (!placed) merged.push_back(cur);
            placed = true;
            merged.push_back(r);
        } else {                                           // overlaps or touches: one range
            cur.begin = std::min(cur.begin, r.begin);
            cur.end = std::max(cur.end, r.end);
        }
    }
    if (!placed) merged.push_back(cur);
    r_.swap(merged);
}

std::vector<UploadSegment> plan_upload(const SlottedRanges& ranges, uint32_t from, uint32_t count, bool reorder) {
    std::vector<UploadSegment> segs;
    for (const SlotCut& c : ranges.cut(from, from + count)) {
        UploadSegment s = {c.begin, c.end, c.fresh || !reorder, 0u, 0u};
        uint32_t lo = c.begin, hi = c.end;
        if (!s.fresh)
            if (const SlotRange* r = ranges.holding(c.begin, c.end - c.begin)) { lo = r->begin; hi = r->end; }
        s.b0 = lo / UPLOAD_BLOCK;
        s.b1 = (hi + UPLOAD_BLOCK - 1u) / UPLOAD_BLOCK;
        segs.push_back(s);
    }
    return segs;
}

UploadLayout upload_layout(uint32_t count, bool cov_half, bool mesh_sh_u8, uint32_t sh_degree, bool source_stages_sh_u8) {
    UploadLayout l;
    l.ncoef = (sh_degree == 0 || (mesh_sh_u8 && !source_stages_sh_u8)) ? 0 : (sh_degree == 1 ? 9 : 24);
    l.sh_u8 = mesh_sh_u8 && l.ncoef != 0;
    const size_t b_c = (size_t)count * 12, b_cov = (size_t)count * (cov_half ? 12 : 24), b_sh = (size_t)count * l.ncoef * (l.sh_u8 ? 1 : 2);
    l.off_cov = (b_c + 255) & ~(size_t)255;
    l.off_sh = (l.off_cov + b_cov + 255) & ~(size_t)255;
    l.off_rgba = (l.off_sh + b_sh + 255) & ~(size_t)255;
    l.bytes = l.off_sh + b_sh + 512 + (size_t)count * 4;
    return l;
}

RemovePlan plan_remove(const std::vector<SlotRange>& runs, const SlottedRanges& slotted, uint32_t uploaded, uint32_t max_count,
                       bool reorder, const uint32_t* ranges, uint32_t n) {
    RemovePlan p;
    if (!ranges || n == 0 || n > REMOVE_MAX_RANGES) { p.refused = "1 .. 32 ranges"; return p; }
    uint64_t prev_end = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t from = ranges[2 * k], end = from + ranges[2 * k + 1];
        if (end == from) { p.refused = "a range is empty"; return p; }
        if (from < prev_end) { p.refused = "the ranges are not ascending and disjoint"; return p; }
        if (end > max_count) { p.refused = "a range exceeds max_splat_count"; return p; }
        prev_end = end;
        if (reorder)
            for (const SlotRange& r : runs)
                if ((r.begin < from && from < r.end) || (r.begin < end && end < r.end)) {
                    p.refused = "a range border falls inside a Morton run (the span of one fresh upload segment)";
                    return p;
                }
        if (from < uploaded) p.cuts.push_back({(uint32_t)from, (uint32_t)std::min<uint64_t>(end, uploaded)});
    }
    // the survivors between and behind the cuts, each with the removed count below it
    uint32_t shift = 0;
    for (size_t k = 0; k < p.cuts.size(); k++) {
        shift += p.cuts[k].end - p.cuts[k].begin;
        const uint32_t stop = k + 1 < p.cuts.size() ? p.cuts[k + 1].begin : uploaded;
        if (p.cuts[k].end < stop) p.moves.push_back({p.cuts[k].end, stop, shift});
    }
    p.removed = shift;
    p.uploaded = uploaded - shift;
    p.first_block = p.cuts.empty() ? 0u : p.cuts[0].begin / UPLOAD_BLOCK;
    // what is left of [b, e), piece by piece, in the new numbering
    auto survivors = [&](uint32_t b, uint32_t e, auto&& emit) {
        uint32_t below = 0, pos = b;                       // below: the removed positions below pos
        for (const SlotRange& c : p.cuts) {
            if (c.begin >= e) break;
            if (c.end > pos) {
                if (c.begin > pos) emit(pos - below, c.begin - below);
                pos = c.end;
            }
            below += c.end - c.begin;
        }
        if (pos < e) emit(pos - below, e - below);
    };
    if (reorder)                                           // (each whole or not at all: one piece; no other mesh has runs)
        for (const SlotRange& r : runs) survivors(r.begin, r.end, [&](uint32_t b, uint32_t e) { p.runs.push_back({b, e}); });
    for (const SlotRange& r : slotted.ranges())
        survivors(r.begin, r.end, [&](uint32_t b, uint32_t e) { p.slotted.add(b, e); });
    return p;
}

ReorderPlan plan_reorder(const std::vector<SlotRange>& runs, const SlottedRanges& slotted, uint32_t uploaded, bool reorder, uint32_t from,
                         uint32_t count) {
    ReorderPlan p;
    if (count == 0) { p.noop = true; return p; }
    const uint64_t end = (uint64_t)from + count;
    if (end > uploaded) { p.refused = "the range exceeds the uploaded splat count"; return p; }
    if (!reorder) { p.noop = true; return p; }            // upload order is kept: there are no runs
    if (!slotted.holding(from, count)) { p.refused = "a position of the range was never uploaded"; return p; }
    uint32_t inside = 0;
    for (const SlotRange& r : runs) {
        if ((r.begin < from && from < r.end) || (r.begin < end && end < r.end)) {
            p.refused = "a range border falls inside a Morton run (the span of one fresh upload segment)";
            return p;
        }
        if (r.begin >= from && r.end <= end) inside++;
    }
    if (inside <= 1) { p.noop = true; return p; }
    bool placed = false;
    for (const SlotRange& r : runs) {
        if (r.begin >= from && r.end <= end) {
            if (!placed) p.runs.push_back({from, (uint32_t)end});
            placed = true;
        } else {
            p.runs.push_back(r);
        }
    }
    p.first_block = from / UPLOAD_BLOCK;
    p.end_block = (uint32_t)((end + UPLOAD_BLOCK - 1u) / UPLOAD_BLOCK);
    return p;
}

// the state of a mesh out of a debug struct's rows; false when no mesh can be in it
static bool debug_state(const uint32_t (*run_rows)[2], uint32_t n_runs, const uint32_t (*slot_rows)[2], uint32_t n_slotted, uint32_t uploaded,
                        std::vector<SlotRange>* runs, SlottedRanges* sl) {
    uint32_t prev = 0;
    for (uint32_t k = 0; k < n_runs; k++) {
        if (run_rows[k][0] >= run_rows[k][1] || run_rows[k][0] < prev || run_rows[k][1] > uploaded) return false;
        runs->push_back({run_rows[k][0], run_rows[k][1]});
        prev = run_rows[k][1];
    }
    for (uint32_t k = 0; k < n_slotted; k++) {
        if (slot_rows[k][0] >= slot_rows[k][1] || slot_rows[k][1] > uploaded) return false;
        sl->add(slot_rows[k][0], slot_rows[k][1]);
    }
    return true;
}

extern "C" int gs_debug_reorder_plan(const gs_reorder_plan_debug_in* in, gs_reorder_plan_debug_out* out) {
    if (!in || !out || in->n_runs > UPLOAD_DEBUG_MAX || in->n_slotted > UPLOAD_DEBUG_MAX || in->uploaded > UPLOAD_MAX_SPLATS) return -1;
    std::vector<SlotRange> runs;
    SlottedRanges sl;
    if (!debug_state(in->runs, in->n_runs, in->slotted, in->n_slotted, in->uploaded, &runs, &sl)) return -1;
    *out = gs_reorder_plan_debug_out();
    const ReorderPlan p = plan_reorder(runs, sl, in->uploaded, in->reorder != 0u, in->from, in->count);
    if (p.refused) { out->refused = 1; return 0; }
    if (p.noop) { out->noop = 1; return 0; }
    out->n_runs = (uint32_t)p.runs.size();                 // (never more than came in)
    for (uint32_t k = 0; k < out->n_runs; k++) { out->runs[k][0] = p.runs[k].begin; out->runs[k][1] = p.runs[k].end; }
    out->first_block = p.first_block; out->end_block = p.end_block;
    return 0;
}

extern "C" int gs_debug_remove_plan(const gs_remove_plan_debug_in* in, gs_remove_plan_debug_out* out) {
    if (!in || !out || in->n_runs > UPLOAD_DEBUG_MAX || in->n_slotted > UPLOAD_DEBUG_MAX || in->n_ranges > UPLOAD_DEBUG_MAX) return -1;
    if (in->max_count > UPLOAD_MAX_SPLATS || in->uploaded > in->max_count) return -1;
    std::vector<SlotRange> runs;
    SlottedRanges sl;
    if (!debug_state(in->runs, in->n_runs, in->slotted, in->n_slotted, in->uploaded, &runs, &sl)) return -1;
    *out = gs_remove_plan_debug_out();
    const RemovePlan p = plan_remove(runs, sl, in->uploaded, in->max_count, in->reorder != 0u, &in->ranges[0][0], in->n_ranges);
    if (p.refused) { out->refused = 1; return 0; }
    if (p.moves.size() > UPLOAD_DEBUG_MAX || p.runs.size() > UPLOAD_DEBUG_MAX || p.slotted.ranges().size() > UPLOAD_DEBUG_MAX) return -1;
    out->n_moves = (uint32_t)p.moves.size();
    for (uint32_t k = 0; k < out->n_moves; k++) {
        out->moves[k][0] = p.moves[k].begin; out->moves[k][1] = p.moves[k].end; out->moves[k][2] = p.moves[k].shift;
    }
    out->n_runs = (uint32_t)p.runs.size();
    for (uint32_t k = 0; k < out->n_runs; k++) { out->runs[k][0] = p.runs[k].begin; out->runs[k][1] = p.runs[k].end; }
    out->n_slotted = (uint32_t)p.slotted.ranges().size();
    for (uint32_t k = 0; k < out->n_slotted; k++) {
        out->slotted[k][0] = p.slotted.ranges()[k].begin; out->slotted[k][1] = p.slotted.ranges()[k].end;
    }
    out->removed = p.removed; out->uploaded = p.uploaded; out->first_block = p.first_block;
    return 0;
}

extern "C" int gs_debug_upload_plan(const gs_upload_plan_debug_in* in, gs_upload_plan_debug_out* out) {
    if (!in || !out || in->n_ranges > UPLOAD_DEBUG_MAX || (uint64_t)in->from + in->count > UPLOAD_MAX_SPLATS) return -1;
    SlottedRanges sl;
    for (uint32_t k = 0; k < in->n_ranges; k++) {
        if (in->ranges[k][0] >= in->ranges[k][1] || in->ranges[k][1] > UPLOAD_MAX_SPLATS) return -1;
        sl.add(in->ranges[k][0], in->ranges[k][1]);
    }
    *out = gs_upload_plan_debug_out();
    auto copy = [](const SlottedRanges& s, uint32_t* n, uint32_t (*rows)[2]) {
        *n = (uint32_t)s.ranges().size();
        for (uint32_t k = 0; k < *n; k++) { rows[k][0] = s.ranges()[k].begin; rows[k][1] = s.ranges()[k].end; }
    };
    copy(sl, &out->n_before, out->before);
    if (const SlotRange* r = sl.holding(in->hold_from, in->hold_count)) { out->held = 1; out->hold_begin = r->begin; out->hold_end = r->end; }
    const std::vector<UploadSegment> segs = plan_upload(sl, in->from, in->count, in->reorder != 0u);
    if (segs.size() > UPLOAD_DEBUG_MAX) return -1;
    out->n_segments = (uint32_t)segs.size();
    for (uint32_t k = 0; k < out->n_segments; k++) {
        const UploadSegment& s = segs[k];
        const uint32_t row[5] = {s.begin, s.end, s.fresh ? 1u : 0u, s.b0, s.b1};
        std::copy(row, row + 5, out->segments[k]);
    }
    sl.add(in->from, in->from + in->count);
    if (sl.ranges().size() > UPLOAD_DEBUG_MAX) return -1;
    copy(sl, &out->n_after, out->after);
    const UploadLayout l = upload_layout(in->layout_count, in->cov_half != 0u, in->mesh_sh_u8 != 0u, in->sh_degree, in->source_stages_sh_u8 != 0u);
    out->ncoef = l.ncoef; out->sh_u8 = l.sh_u8 ? 1u : 0u;
    out->off_cov = l.off_cov; out->off_sh = l.off_sh; out->off_rgba = l.off_rgba; out->bytes = l.bytes;
    return 0;
}
