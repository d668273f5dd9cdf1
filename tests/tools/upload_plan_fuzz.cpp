// tests/tools/upload_plan_fuzz.cpp — a stand-alone program over csrc/upload_plan.cpp (host only: nothing of HIP) for a sanitizer
// run by hand: the upload's host policy on the inputs of the test cases (`python tests/upload_plan_cases.py dump cases.bin`) and on
// seeded random sequences of uploads into meshes of a few thousand splats, against a brute-force bitmap of the slotted splats.
// After every upload: the ranges are the bitmap's runs; the segments tile [from, end) without gap or overlap; each segment's bits
// are all clear or all set, as `fresh` says; holding() equals the brute-force answer; the box spans are the model's (a fresh
// segment's own blocks, else those of the run that held it).  It prints one summary line; a sanitizer report or a failed check is
// what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/upload_plan_fuzz.cpp gaussiansplats3d_amd/csrc/upload_plan.cpp -o upload_plan_fuzz && \
//       ./upload_plan_fuzz cases.bin 2000 1
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

// the run of set bits around [from, from + count), by walking the bitmap (count >= 1); false: some bit is clear or beyond the mesh
static bool brute_holding(const std::vector<uint8_t>& bits, uint64_t from, uint64_t count, uint32_t* begin, uint32_t* end) {
    if (from + count > bits.size()) return false;
    for (uint64_t i = from; i < from + count; i++)
        if (!bits[i]) return false;
    uint64_t b = from, e = from + count;
    while (b > 0 && bits[b - 1]) b--;
    while (e < bits.size() && bits[e]) e++;
    *begin = (uint32_t)b; *end = (uint32_t)e;
    return true;
}

static void check_ranges(const SlottedRanges& sl, const std::vector<uint8_t>& bits) {
    std::vector<SlotRange> runs;
    for (size_t i = 0; i < bits.size(); i++)
        if (bits[i] && (i == 0 || !bits[i - 1])) {
            size_t e = i;
            while (e < bits.size() && bits[e]) e++;
            runs.push_back({(uint32_t)i, (uint32_t)e});
        }
    const std::vector<SlotRange>& r = sl.ranges();
    CHECK(r.size() == runs.size());
    for (size_t k = 0; k < std::min(r.size(), runs.size()); k++) CHECK(r[k].begin == runs[k].begin && r[k].end == runs[k].end);
}

// one upload into (sl, bits), checked; the plan lives in an exact-size heap block
static void upload(SlottedRanges& sl, std::vector<uint8_t>& bits, uint32_t from, uint32_t count, bool reorder, uint64_t* digest) {
    const std::vector<UploadSegment> plan = plan_upload(sl, from, count, reorder);
    std::unique_ptr<UploadSegment[]> segs(new UploadSegment[plan.size() ? plan.size() : 1]);
    std::copy(plan.begin(), plan.end(), segs.get());
    uint32_t pos = from;
    for (size_t k = 0; k < plan.size(); k++) {
        const UploadSegment& s = segs[k];
        CHECK(s.begin == pos && s.end > s.begin && s.end <= from + count);
        if (s.end <= s.begin || s.end > bits.size()) break;
        pos = s.end;
        bool any = false, all = true;
        for (uint32_t i = s.begin; i < s.end; i++) { any = any || bits[i]; all = all && bits[i]; }
        CHECK(any == all);                                   // all clear or all set ...
        CHECK(s.fresh == (!any || !reorder));                // ... as `fresh` says (always fresh when the mesh keeps upload order)
        CHECK(k == 0 || !reorder || segs[k - 1].fresh != s.fresh);   // cut only where the bits change
        uint32_t lo = s.begin, hi = s.end;
        if (!s.fresh) CHECK(brute_holding(bits, s.begin, s.end - s.begin, &lo, &hi));
        CHECK(s.b0 == lo / 256u && s.b1 == (hi + 255u) / 256u && s.b0 < s.b1);
        mix(digest, s.begin + ((uint64_t)s.end << 20) + ((uint64_t)s.b0 << 40) + ((uint64_t)s.b1 << 50) + ((uint64_t)s.fresh << 63));
    }
    CHECK(pos == from + count);
    sl.add(from, from + count);
    for (uint32_t i = from; i < from + count; i++) bits[i] = 1;
    check_ranges(sl, bits);
    mix(digest, sl.ranges().size());
}

static void check_holding(const SlottedRanges& sl, const std::vector<uint8_t>& bits, uint32_t from, uint32_t count) {
    uint32_t b = 0, e = 0;
    const SlotRange* r = sl.holding(from, count);
    const bool want = brute_holding(bits, from, count, &b, &e);
    CHECK((r != nullptr) == want);
    if (r && want) CHECK(r->begin == b && r->end == e);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: upload_plan_fuzz <cases.bin | -> [random sequences] [seed]\n"); return 2; }
    const long sequences = argc > 2 ? atol(argv[2]) : 2000;
    const unsigned seed = argc > 3 ? (unsigned)atol(argv[3]) : 1u;
    uint64_t digest = 1469598103934665603ull;
    long from_file = 0, uploads = 0, held = 0;
    if (strcmp(argv[1], "-") != 0) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("%s: cannot be read\n", argv[1]); return 2; }
        std::unique_ptr<gs_upload_plan_debug_in> in(new gs_upload_plan_debug_in());
        std::unique_ptr<gs_upload_plan_debug_out> out(new gs_upload_plan_debug_out());
        while (fread(in.get(), sizeof(*in), 1, f) == 1) {
            CHECK(gs_debug_upload_plan(in.get(), out.get()) == 0);
            CHECK(out->n_segments <= UPLOAD_DEBUG_MAX && out->n_after <= UPLOAD_DEBUG_MAX && (in->count == 0) == (out->n_segments == 0));
            for (uint32_t k = 0; k < out->n_segments; k++) {
                const uint32_t* s = out->segments[k];
                CHECK(s[0] == (k ? out->segments[k - 1][1] : in->from) && s[1] > s[0] && s[3] <= s[0] / 256u && s[4] >= (s[1] + 255u) / 256u);
            }
            if (out->n_segments) CHECK(out->segments[out->n_segments - 1][1] == in->from + in->count);
            CHECK(out->off_cov % 256 == 0 && out->off_sh % 256 == 0 && out->off_rgba % 256 == 0 && out->off_rgba + 4ull * in->layout_count <= out->bytes);
            mix(&digest, out->n_segments + 256ull * out->n_after + 65536ull * out->held + (out->bytes << 24));
            from_file++;
        }
        fclose(f);
    }
    std::mt19937 rng(seed);
    auto u = [&](uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; };
    for (long q = 0; q < sequences; q++) {
        const uint32_t n = u(4) == 0 ? 1u + u(600) : 2000u + u(3000);          // splats of this mesh
        const bool reorder = u(4) != 0;
        std::vector<uint8_t> bits(n, 0);
        SlottedRanges sl;
        const uint32_t steps = 1u + u(24);
        for (uint32_t s = 0; s < steps; s++) {
            // short spans, spans that start or end on a border of a range or of a block, whole-mesh spans
            uint32_t a = u(n + 1), b = u(n + 1);
            if (u(3) == 0 && !sl.ranges().empty()) {
                const SlotRange& r = sl.ranges()[u((uint32_t)sl.ranges().size())];
                a = u(2) ? r.begin : r.end;
            }
            if (u(4) == 0) b = std::min(n, a + u(40));
            if (u(6) == 0) a = std::min(n, (a / 256u) * 256u);
            if (u(6) == 0) b = std::min(n, (b / 256u) * 256u);
            if (u(16) == 0) { a = 0; b = n; }
            const uint32_t from = std::min(a, b), count = std::max(a, b) - from;
            upload(sl, bits, from, count, reorder, &digest);
            uploads++;
            for (int h = 0; h < 4; h++) {
                uint32_t hf = u(n + 2), hc = 1u + u(u(2) ? 50u : n);
                if (u(8) == 0) { hf = 0xFFFFFFFFu - u(64); hc = (0xFFFFFFFFu - hf) + 1u + u(n + 1u); }   // from + count wraps to 0 .. n in 32 bits
                check_holding(sl, bits, hf, hc);
                held += sl.holding(hf, hc) != nullptr;
            }
            if (!sl.ranges().empty()) {                      // a range is held by itself, and not with one splat more on either side
                const SlotRange r = sl.ranges()[u((uint32_t)sl.ranges().size())];
                check_holding(sl, bits, r.begin, r.end - r.begin);
                check_holding(sl, bits, r.begin, r.end - r.begin + 1u);
                if (r.begin) check_holding(sl, bits, r.begin - 1u, r.end - r.begin + 1u);
            }
        }
    }
    printf("upload_plan_fuzz: %ld case inputs, %ld random sequences, %ld uploads (seed %u, %ld spans held), digest %016llx, %d failed checks\n",
           from_file, sequences, uploads, seed, held, (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
