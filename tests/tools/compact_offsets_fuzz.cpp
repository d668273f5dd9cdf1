// tests/tools/compact_offsets_fuzz.cpp — a stand-alone program over csrc/extreme_set.cpp (host only: nothing of HIP) for a sanitizer
// run by hand: the 16-bit-centre-plane decision (gs_compact_offsets) over the extreme set of seeded random clouds - boxes of every
// width around 2^16, anywhere in int32 and at its two ends, appended origins, empty and one-row sets - held to brute force over ALL
// points in int64.  The rows live in exact-size heap blocks, so a read past the set is a report.  It prints one summary line; a
// sanitizer report or a failed check is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/compact_offsets_fuzz.cpp gaussiansplats3d_amd/csrc/extreme_set.cpp -o compact_offsets_fuzz && ./compact_offsets_fuzz 2000 1
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>
#include <vector>

#include "extreme_set.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 10) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

int main(int argc, char** argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 0) : 1);
    auto uniform = [&](int64_t lo, int64_t hi) { return std::uniform_int_distribution<int64_t>(lo, hi)(rng); };
    int fit = 0, wide = 0, none = 0;
    int32_t off[3] = {1, 2, 3};
    CHECK(!gs_compact_offsets(nullptr, 0, off) && off[0] == 1 && off[1] == 2 && off[2] == 3);
    CHECK(gs_debug_compact_offsets(nullptr, 0, nullptr) == -1 && gs_debug_compact_offsets(nullptr, 3, off) == -1);
    for (int it = 0; it < iterations; it++) {
        const size_t n = (size_t)uniform(1, it % 50 == 0 ? 20000 : 600);
        int64_t base[3], width[3];
        for (int k = 0; k < 3; k++) {
            const int64_t w = uniform(0, 9);
            width[k] = w < 5 ? uniform(0, 65535) : (w < 7 ? 65535 + uniform(-2, 2) : (w < 9 ? uniform(65536, 200000) : uniform(0, 4294967295LL)));
            const int64_t lo_min = INT32_MIN, lo_max = (int64_t)INT32_MAX - width[k];
            const int64_t where = uniform(0, 3);
            base[k] = where == 0 ? lo_min : (where == 1 ? lo_max : uniform(lo_min, lo_max));
        }
        std::unique_ptr<int32_t[]> rows(new int32_t[n * 4]);
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 3; k++) rows[4 * i + k] = (int32_t)(base[k] + uniform(0, width[k]));
            rows[4 * i + 3] = (int32_t)uniform(INT32_MIN, INT32_MAX);
        }
        const bool origin = it % 7 == 0;                       // a zero-filled tail: the point (0, 0, 0) joins the set
        std::vector<int32_t> set, grown;
        if (!gs_extreme_set(nullptr, 0, rows.get(), n, GS_EXTREME_CAP, set)) { none++; continue; }
        if (origin) {
            const int32_t zero[4] = {0, 0, 0, 0};
            if (!gs_extreme_set(set.data(), set.size() / 4, zero, 1, GS_EXTREME_CAP, grown)) { none++; continue; }
            set.swap(grown);
        }
        int64_t lo[3], hi[3];
        for (int k = 0; k < 3; k++) lo[k] = hi[k] = origin ? 0 : rows[k];
        for (size_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) {
                lo[k] = std::min<int64_t>(lo[k], rows[4 * i + k]);
                hi[k] = std::max<int64_t>(hi[k], rows[4 * i + k]);
            }
        const bool want = hi[0] - lo[0] <= 65535 && hi[1] - lo[1] <= 65535 && hi[2] - lo[2] <= 65535;
        std::unique_ptr<int32_t[]> exact(new int32_t[set.size()]);          // exact size: the last row ends the block
        std::copy(set.begin(), set.end(), exact.get());
        std::unique_ptr<int32_t[]> o(new int32_t[3]);
        o[0] = o[1] = o[2] = 0x5A5A5A5A;
        const bool got = gs_compact_offsets(exact.get(), set.size() / 4, o.get());
        CHECK(got == want);
        if (got) {
            CHECK(o[0] == lo[0] && o[1] == lo[1] && o[2] == lo[2]);
            for (size_t i = 0; i < n; i++)
                for (int k = 0; k < 3; k++) {
                    const int64_t d = (int64_t)rows[4 * i + k] - o[k];
                    CHECK(d >= 0 && d <= 65535);
                }
        } else {
            CHECK(o[0] == 0x5A5A5A5A && o[1] == 0x5A5A5A5A && o[2] == 0x5A5A5A5A);
        }
        CHECK(gs_debug_compact_offsets(exact.get(), (uint32_t)(set.size() / 4), o.get()) == (want ? 1 : 0));
        (got ? fit : wide)++;
    }
    printf("compact_offsets_fuzz: %d inputs, %d fit, %d too wide, %d without a set, %d failures\n", iterations, fit, wide, none, failures);
    return failures ? 1 : 0;
}
