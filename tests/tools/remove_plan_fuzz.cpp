// tests/tools/remove_plan_fuzz.cpp — a stand-alone program over csrc/upload_plan.cpp (host only: nothing of HIP) for a sanitizer
// run by hand: plan_remove on seeded random meshes of a few thousand positions - random uploads build the runs and the slotted
// ranges, random removals (whole runs, pieces of holes, anything on a mesh that keeps upload order, malformed calls) edit them -
// against brute-force vectors: per position "owns a slot", its run number and "goes away".  After every accepted removal: the moves
// are exactly the survivors whose position changes, each with the removed count below it; the runs and slotted ranges are what the
// vectors say; uploaded and first_block follow.  A refusal must be one the vectors explain.  The debug entry is driven with the
// same inputs.  It prints one summary line; a sanitizer report or a failed check is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/remove_plan_fuzz.cpp gaussiansplats3d_amd/csrc/upload_plan.cpp -o remove_plan_fuzz && ./remove_plan_fuzz 2000 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
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

// the ranges of a vector's maximal stretches with the same non-zero value
template <class T>
static std::vector<SlotRange> stretches(const std::vector<T>& v) {
    std::vector<SlotRange> out;
    for (size_t i = 0; i < v.size();) {
        size_t e = i + 1;
        while (e < v.size() && v[e] == v[i]) e++;
        if (v[i]) out.push_back({(uint32_t)i, (uint32_t)e});
        i = e;
    }
    return out;
}
static bool same(const std::vector<SlotRange>& a, const std::vector<SlotRange>& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k].begin != b[k].begin || a[k].end != b[k].end) return false;
    return true;
}

static void remove_once(Model& m, const std::vector<uint32_t>& pairs, uint64_t* digest, uint32_t* accepted, uint32_t* refused) {
    const uint32_t n = (uint32_t)(pairs.size() / 2);
    std::unique_ptr<uint32_t[]> exact(new uint32_t[pairs.size() ? pairs.size() : 1]);   // an exact-size block: reads past n pairs show
    std::copy(pairs.begin(), pairs.end(), exact.get());
    const RemovePlan p = plan_remove(m.runs, m.sl, m.uploaded, m.cap, m.reorder, exact.get(), n);
    // the brute-force verdict
    bool ok = n >= 1 && n <= REMOVE_MAX_RANGES;
    std::vector<uint8_t> gone(m.cap, 0);
    uint64_t prev = 0;
    for (uint32_t k = 0; ok && k < n; k++) {
        const uint64_t b = pairs[2 * k], e = b + pairs[2 * k + 1];
        if (e == b || b < prev || e > m.cap) { ok = false; break; }
        prev = e;
        for (uint64_t i = b; i < e; i++) gone[i] = 1;
    }
    if (ok && m.reorder)
        for (uint32_t k = 0; k < 2 * n; k++) {                 // neither border of a range has the same run on both sides
            const uint64_t at = k & 1u ? (uint64_t)pairs[k - 1] + pairs[k] : pairs[k];
            if (at > 0 && at < m.cap && m.run[at - 1] && m.run[at - 1] == m.run[at]) ok = false;
        }
    CHECK(ok == (p.refused == nullptr));
    gs_remove_plan_debug_in in = {};
    gs_remove_plan_debug_out out = {};
    const bool fits = m.runs.size() <= UPLOAD_DEBUG_MAX && m.sl.ranges().size() <= UPLOAD_DEBUG_MAX && n <= UPLOAD_DEBUG_MAX;
    if (fits) {
        in.n_runs = (uint32_t)m.runs.size();
        for (uint32_t k = 0; k < in.n_runs; k++) { in.runs[k][0] = m.runs[k].begin; in.runs[k][1] = m.runs[k].end; }
        in.n_slotted = (uint32_t)m.sl.ranges().size();
        for (uint32_t k = 0; k < in.n_slotted; k++) { in.slotted[k][0] = m.sl.ranges()[k].begin; in.slotted[k][1] = m.sl.ranges()[k].end; }
        in.uploaded = m.uploaded; in.max_count = m.cap; in.reorder = m.reorder ? 1u : 0u; in.n_ranges = n;
        for (uint32_t k = 0; k < n; k++) { in.ranges[k][0] = pairs[2 * k]; in.ranges[k][1] = pairs[2 * k + 1]; }
        const int st = gs_debug_remove_plan(&in, &out);
        CHECK(st == 0 || (ok && (p.moves.size() > UPLOAD_DEBUG_MAX || p.runs.size() > UPLOAD_DEBUG_MAX || p.slotted.ranges().size() > UPLOAD_DEBUG_MAX)));
        if (st == 0) CHECK((out.refused != 0u) == !ok);
    }
    if (!ok || p.refused) { (*refused)++; return; }
    (*accepted)++;
    for (uint32_t i = m.uploaded; i < m.cap; i++) gone[i] = 0;            // positions beyond the uploaded count were never there
    std::vector<uint8_t> slot2;
    std::vector<uint32_t> run2;
    std::vector<uint32_t> shift_of(m.uploaded, 0);
    uint32_t removed = 0, first_gone = m.cap;
    for (uint32_t i = 0; i < m.uploaded; i++) {
        if (gone[i]) { removed++; first_gone = std::min(first_gone, i); continue; }
        shift_of[i] = removed;
        slot2.push_back(m.slot[i]);
        run2.push_back(m.reorder ? m.run[i] : 0u);
    }
    CHECK(p.removed == removed && p.uploaded == m.uploaded - removed);
    if (removed) CHECK(p.first_block == first_gone / UPLOAD_BLOCK);
    // every survivor that moves is in exactly one move, with its own shift; nothing else is in any
    std::vector<uint32_t> covered(m.uploaded, 0);
    uint32_t last_end = 0;
    for (const RemoveMove& mv : p.moves) {
        CHECK(mv.begin < mv.end && mv.end <= m.uploaded && mv.shift > 0 && mv.begin >= last_end);
        last_end = mv.end;
        for (uint32_t i = mv.begin; i < mv.end && i < m.uploaded; i++) { covered[i] = mv.shift; CHECK(!gone[i]); }
    }
    for (uint32_t i = 0; i < m.uploaded; i++) CHECK(covered[i] == (gone[i] ? 0u : shift_of[i]));
    CHECK(same(p.runs, stretches(run2)));
    CHECK(same(p.slotted.ranges(), stretches(slot2)));
    if (fits && out.refused == 0u) {
        CHECK(out.n_moves == p.moves.size() && out.n_runs == p.runs.size() && out.n_slotted == p.slotted.ranges().size());
        CHECK(out.removed == p.removed && out.uploaded == p.uploaded && out.first_block == p.first_block);
    }
    // the state the next call sees
    slot2.resize(m.cap, 0); run2.resize(m.cap, 0);
    m.slot.swap(slot2); m.run.swap(run2);
    m.sl = p.slotted; m.runs = p.runs; m.uploaded = p.uploaded;
    mix(digest, p.removed); mix(digest, p.moves.size()); mix(digest, p.runs.size());
}

int main(int argc, char** argv) {
    const uint32_t rounds = argc > 1 ? (uint32_t)atoi(argv[1]) : 2000u;
    std::mt19937 rng(argc > 2 ? (uint32_t)atoi(argv[2]) : 1u);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (uint64_t)(hi - lo + 1u)); };
    uint64_t digest = 1469598103934665603ull;
    uint32_t accepted = 0, refused = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        Model m;
        m.cap = pick(1, 3000);
        m.reorder = pick(0, 3) != 0;
        m.slot.assign(m.cap, 0); m.run.assign(m.cap, 0);
        for (uint32_t u = pick(0, 6); u > 0; u--) {
            const uint32_t from = pick(0, m.cap - 1);
            upload(m, from, pick(1, std::min(m.cap - from, 900u)));
        }
        for (uint32_t e = pick(1, 4); e > 0; e--) {
            std::vector<uint32_t> pairs;
            const uint32_t style = pick(0, 9);
            if (style <= 4 && !m.runs.empty()) {                   // whole runs (and sometimes a hole beside one)
                uint32_t at = 0;
                for (const SlotRange& run : m.runs)
                    if (pick(0, 2) == 0 && run.begin >= at && pairs.size() < 2 * REMOVE_MAX_RANGES) {
                        const uint32_t b = pick(0, 3) == 0 ? pick(at, run.begin) : run.begin;
                        bool clean = true;                         // (the hole piece must not cut an earlier run)
                        for (const SlotRange& o : m.runs) clean = clean && !(o.begin < b && b < o.end);
                        const uint32_t begin = clean ? b : run.begin;
                        pairs.push_back(begin); pairs.push_back(run.end - begin);
                        at = run.end;
                    }
            } else if (style <= 8) {                               // anything ascending
                uint32_t at = 0;
                for (uint32_t k = pick(0, 5); k > 0 && at < m.cap; k--) {
                    const uint32_t b = pick(at, std::min(m.cap - 1, at + 400u)), c = pick(1, std::min(m.cap - b, 300u));
                    pairs.push_back(b); pairs.push_back(c);
                    at = b + c;
                }
            } else {                                               // malformed: empty, descending, too long, too many, wrapping
                const uint32_t kind = pick(0, 4);
                if (kind == 0) pairs = {pick(0, m.cap), 0u};
                else if (kind == 1) pairs = {m.cap / 2u, 1u, 0u, 1u};
                else if (kind == 2) pairs = {pick(0, m.cap), m.cap + 1u};
                else if (kind == 3) for (uint32_t k = 0; k < 33; k++) { pairs.push_back(k); pairs.push_back(1u); }
                else pairs = {0xFFFFFFF0u, 0x20u};
            }
            remove_once(m, pairs, &digest, &accepted, &refused);
            if (pick(0, 2) == 0 && m.cap > 0) {                    // and an upload in between: a new run behind or into the survivors
                const uint32_t from = pick(0, m.cap - 1);
                upload(m, from, pick(1, std::min(m.cap - from, 500u)));
            }
        }
    }
    printf("remove_plan_fuzz: %u rounds, %u removals accepted, %u refused, digest %016llx, %d failures\n", rounds, accepted, refused,
           (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
