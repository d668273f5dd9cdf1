// tests/tools/reorder_plan_fuzz.cpp — a stand-alone program over csrc/upload_plan.cpp (host only: nothing of HIP) for a sanitizer
// run by hand: plan_reorder on seeded random meshes of a few thousand positions - random uploads build the runs and the slotted
// ranges, random folds (whole runs, borders inside runs, holes, ranges beyond the uploaded count, a mesh that keeps upload order)
// edit them - against brute-force vectors: per position "owns a slot" and its run number.  Every verdict (refused / nothing to do /
// folded) must be the one the vectors give; after a fold the runs are what the vectors say and the blocks follow.  The debug entry
// is driven with the same inputs.  It prints one summary line; a sanitizer report or a failed check is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/reorder_plan_fuzz.cpp gaussiansplats3d_amd/csrc/upload_plan.cpp -o reorder_plan_fuzz && ./reorder_plan_fuzz 2000 1
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "upload_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 10) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

static void mix(uint64_t* digest, uint64_t v) { *digest = (*digest ^ v) * 1099511628211ull; }

struct Model {
    uint32_t cap = 0, uploaded = 0;
    bool reorder = true;
    std::vector<uint8_t> slot;         // per position
    std::vector<uint32_t> run;         // 0: none
    uint32_t next_run = 1;
    SlottedRanges sl;
    std::vector<SlotRange> runs;
};

static void upload(Model& m, uint32_t from, uint32_t count) {
    for (const UploadSegment& s : plan_upload(m.sl, from, count, m.reorder)) {
        if (m.reorder && s.fresh) {
            m.runs.insert(std::upper_bound(m.runs.begin(), m.runs.end(), s.begin, [](uint32_t b, const SlotRange& r) { return b < r.begin; }),
                          SlotRange{s.begin, s.end});
            for (uint32_t i = s.begin; i < s.end; i++) m.run[i] = m.next_run;
            m.next_run++;
        }
    }
    for (uint32_t i = from; i < from + count; i++) m.slot[i] = 1;
    m.sl.add(from, from + count);
    m.uploaded = std::max(m.uploaded, from + count);
}

// the maximal stretches of one non-zero run number
static std::vector<SlotRange> stretches(const std::vector<uint32_t>& v) {
    std::vector<SlotRange> out;
    for (size_t i = 0; i < v.size();) {
        size_t e = i + 1;
        while (e < v.size() && v[e] == v[i]) e++;
        if (v[i]) out.push_back({(uint32_t)i, (uint32_t)e});
        i = e;
    }
    return out;
}

enum Verdict { REFUSED, NOOP, FOLDED };

static void fold_once(Model& m, uint32_t from, uint32_t count, uint64_t* digest, uint32_t counts[3]) {
    const ReorderPlan p = plan_reorder(m.runs, m.sl, m.uploaded, m.reorder, from, count);
    const uint64_t end = (uint64_t)from + count;
    // the verdict of the vectors
    Verdict want = FOLDED;
    if (count == 0) want = NOOP;
    else if (end > m.uploaded) want = REFUSED;
    else if (!m.reorder) want = NOOP;
    else {
        bool hole = false;
        std::set<uint32_t> inside;
        for (uint32_t i = from; i < end; i++) {
            hole = hole || !m.slot[i];
            if (m.run[i]) inside.insert(m.run[i]);
        }
        const bool split_begin = from > 0 && m.run[from - 1] && m.run[from - 1] == m.run[from];
        const bool split_end = end < m.cap && m.run[end - 1] && m.run[end - 1] == m.run[end];
        if (hole || split_begin || split_end) want = REFUSED;
        else if (inside.size() <= 1) want = NOOP;
    }
    const Verdict got = p.refused ? REFUSED : (p.noop ? NOOP : FOLDED);
    CHECK(got == want);
    CHECK(!(p.refused && p.noop));
    counts[got]++;
    mix(digest, got);

    gs_reorder_plan_debug_in in = {};
    gs_reorder_plan_debug_out out = {};
    const bool fits = m.runs.size() <= UPLOAD_DEBUG_MAX && m.sl.ranges().size() <= UPLOAD_DEBUG_MAX;
    if (fits) {
        in.n_runs = (uint32_t)m.runs.size();
        for (uint32_t k = 0; k < in.n_runs; k++) { in.runs[k][0] = m.runs[k].begin; in.runs[k][1] = m.runs[k].end; }
        in.n_slotted = (uint32_t)m.sl.ranges().size();
        for (uint32_t k = 0; k < in.n_slotted; k++) { in.slotted[k][0] = m.sl.ranges()[k].begin; in.slotted[k][1] = m.sl.ranges()[k].end; }
        in.uploaded = m.uploaded; in.reorder = m.reorder ? 1u : 0u; in.from = from; in.count = count;
        CHECK(gs_debug_reorder_plan(&in, &out) == 0);
        CHECK((out.refused != 0u) == (got == REFUSED) && (out.noop != 0u) == (got == NOOP));
    }
    if (got != FOLDED || want != FOLDED) return;
    for (uint32_t i = from; i < end; i++) m.run[i] = m.next_run;
    m.next_run++;
    const std::vector<SlotRange> runs = stretches(m.run);
    CHECK(runs.size() == p.runs.size());
    for (size_t k = 0; k < runs.size() && k < p.runs.size(); k++) CHECK(runs[k].begin == p.runs[k].begin && runs[k].end == p.runs[k].end);
    CHECK(p.first_block == from / UPLOAD_BLOCK && (uint64_t)p.end_block * UPLOAD_BLOCK >= end && (uint64_t)(p.end_block - 1u) * UPLOAD_BLOCK < end);
    if (fits) {
        CHECK(out.n_runs == p.runs.size() && out.first_block == p.first_block && out.end_block == p.end_block);
        for (uint32_t k = 0; k < out.n_runs && k < p.runs.size(); k++) CHECK(out.runs[k][0] == p.runs[k].begin && out.runs[k][1] == p.runs[k].end);
    }
    m.runs = p.runs;
    mix(digest, p.runs.size()); mix(digest, p.first_block); mix(digest, p.end_block);
}

int main(int argc, char** argv) {
    const uint32_t rounds = argc > 1 ? (uint32_t)atoi(argv[1]) : 500;
    const uint32_t seed = argc > 2 ? (uint32_t)atoi(argv[2]) : 1;
    std::mt19937 rng(seed);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1u)); };
    uint64_t digest = 1469598103934665603ull;
    uint32_t counts[3] = {0, 0, 0};
    for (uint32_t r = 0; r < rounds; r++) {
        Model m;
        m.cap = pick(1, 3000);
        m.reorder = pick(0, 7) != 0;
        m.slot.assign(m.cap, 0);
        m.run.assign(m.cap, 0);
        const uint32_t uploads = pick(1, 30);
        uint32_t at = pick(0, 3) == 0 ? pick(0, m.cap - 1) : 0;
        for (uint32_t u = 0; u < uploads && at < m.cap; u++) {         // mostly one behind the other, sometimes a hole or a re-upload
            const uint32_t count = pick(1, std::min(m.cap - at, 400u));
            upload(m, at, count);
            const uint32_t kind = pick(0, 9);
            at = kind == 0 ? at + count + pick(1, 50) : (kind == 1 ? pick(0, at + count - 1) : at + count);
        }
        for (uint32_t f = 0; f < 12; f++) {
            uint32_t from, count;
            const uint32_t kind = pick(0, 5);
            if (kind <= 2 && m.runs.size() >= 1) {                      // run borders
                const uint32_t a = pick(0, (uint32_t)m.runs.size() - 1), b = pick(a, std::min<uint32_t>((uint32_t)m.runs.size() - 1, a + 6));
                from = m.runs[a].begin;
                count = m.runs[b].end - from;
                if (kind == 2) { from += pick(0, 1); count -= std::min(count, pick(0, 1)); }
            } else if (kind == 3) {                                     // anything, also beyond the uploaded count
                from = pick(0, m.cap + 10);
                count = pick(0, m.cap + 10);
            } else if (kind == 4) {
                from = 0xFFFFFFF0u; count = pick(0, 0x40);
            } else {
                from = pick(0, m.uploaded ? m.uploaded - 1 : 0);
                count = pick(0, m.uploaded - from);
            }
            fold_once(m, from, count, &digest, counts);
        }
    }
    printf("reorder_plan_fuzz: %u rounds, %u folds, %u with nothing to do, %u refused, digest %016llx, %d failures\n", rounds, counts[FOLDED],
           counts[NOOP], counts[REFUSED], (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
