// tests/tools/sort_plan_fuzz.cpp — a stand-alone program over csrc/sort_plan.cpp and csrc/extreme_set.cpp (host only: nothing of
// HIP) for a sanitizer run by hand: the sort's host policy on the inputs of the test cases (`python tests/sort_plan_cases.py dump
// cases.bin`) and on seeded random inputs - zero counts, counts beyond `uploaded`, sort_count > render_count, precisions 0 .. 40,
// clean_slot and enum words out of range, cu_count 0, every switch - with the key range of random extreme sets and coefficients
// (gs_key_range) as the plan's range.  It checks what must hold for ANY input and prints one summary line; a sanitizer report or a
// failed check is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/sort_plan_fuzz.cpp gaussiansplats3d_amd/csrc/sort_plan.cpp gaussiansplats3d_amd/csrc/extreme_set.cpp \
//       -o sort_plan_fuzz && ./sort_plan_fuzz cases.bin 100000 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <vector>

#include "../../include/gsplat_hip.h"
#include "extreme_set.hpp"
#include "sort_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 10) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// one input through the debug entry; the input and the plan live in exact-size heap blocks
static void run(const SortPlanIn& src, uint64_t* digest) {
    std::unique_ptr<SortPlanIn> in(new SortPlanIn(src));
    std::unique_ptr<SortPlan> out(new SortPlan());
    CHECK(gs_debug_sort_plan(in.get(), out.get()) == 0);
    const SortPlan& pl = *out;
    const uint32_t precision = std::min(in->precision, 32u);
    CHECK(pl.R <= in->uploaded && pl.Rs <= pl.R && pl.sort_start == pl.R - pl.Rs);
    CHECK(pl.val_bits >= 1 && pl.val_bits <= 32 && (pl.val_bits == 32 || pl.max_payload < (1u << pl.val_bits)));
    CHECK(pl.max_payload >= pl.last_splat);
    CHECK(!(pl.cull && pl.vis_cull));
    CHECK(pl.gather <= SORT_GATHER_FUSED && (pl.gather == SORT_GATHER_NONE) == !(in->list == SORT_LIST_DEVICE && in->pending_gather));
    // exactly one front end - none only when nothing is sorted
    CHECK(pl.front < SORT_FRONT_KINDS && (pl.front == SORT_FRONT_NONE) == (pl.Rs == 0));
    const bool known = pl.front == SORT_FRONT_KNOWN_WIDE || pl.front == SORT_FRONT_KNOWN_NARROW || pl.front == SORT_FRONT_KNOWN_COMPACT;
    const bool narrow = pl.front == SORT_FRONT_KNOWN_NARROW || pl.front == SORT_FRONT_KNOWN_COMPACT;
    const bool tree = pl.front == SORT_FRONT_TREE || pl.front == SORT_FRONT_TREE_CULL;
    const bool vis = pl.front == SORT_FRONT_VIS_STREAM || pl.front == SORT_FRONT_VIS_COMPACT;
    CHECK(known == (pl.known_range != 0));
    CHECK(sort_wants_key_range(*in) || !known);
    // known range => identity list, no cull, static integer, sort_start == 0, R == uploaded > 0
    CHECK(!known || (in->list == SORT_LIST_IDENTITY && !pl.cull && !pl.vis_cull && !in->count_on_device && in->flags == GS_SORT_INTEGER &&
                     !in->precomputed && pl.sort_start == 0 && pl.R == in->uploaded && pl.R > 0 && in->range_ok && in->extreme_current &&
                     !in->sw.no_known_range && pl.range_lo == in->range_lo && pl.range_hi == in->range_hi));
    CHECK(known || (pl.range_lo == 0 && pl.range_hi == 0));
    CHECK(!narrow || (known && in->precision <= 16));                                      // narrow => known range and precision <= 16
    CHECK(pl.front != SORT_FRONT_KNOWN_COMPACT || (narrow && in->c16_current));            // compact => narrow
    CHECK(tree == (pl.gather == SORT_GATHER_FUSED && pl.Rs > 0) && (pl.gather != SORT_GATHER_FUSED || pl.Rs > 0));
    CHECK(!vis || pl.vis_cull);
    CHECK(pl.own_payloads == (uint32_t)(tree || pl.front == SORT_FRONT_VIS_STREAM));
    // every grid is >= 1 and within its table
    const uint32_t cus2 = std::max(in->cu_count, 1u) * 2u;
    if (pl.Rs > 0 && !known && !tree) CHECK(pl.front_grid >= 1 && pl.front_grid <= cus2 * 2u);
    if (vis) {
        CHECK(pl.front_grid <= cus2 && (uint64_t)pl.front_grid * pl.front_len >= pl.R && pl.counts_words >= pl.front_grid);
        CHECK(!pl.vis_derive || (pl.derive_grid >= 1 && pl.derive_grid <= cus2 && (uint64_t)pl.derive_grid * pl.derive_len >= pl.R &&
                                 pl.counts_words >= pl.derive_grid * VC_DERIVE_SUBS));
        CHECK((pl.front == SORT_FRONT_VIS_COMPACT) == (pl.key_grid != 0));
    }
    // the passes
    CHECK(pl.passes == (pl.Rs > 0 ? (precision + 7) / 8 : 0u) && pl.passes <= (uint32_t)RADIX_MAX_PASSES);
    if (pl.Rs > 0) {
        CHECK((pl.pass0_slot == 0 || pl.pass0_slot == 3) && (pl.next_clean_slot == 0 || pl.next_clean_slot == 3) &&
              pl.next_clean_slot != pl.pass0_slot);
        CHECK(pl.pass0_slot == 0 || known);
    } else {
        CHECK(pl.next_clean_slot == in->clean_slot);
    }
    bool packed = false;
    for (uint32_t p = 0; p < pl.passes; p++) {
        const SortPass& ps = pl.pass[p];
        const bool last = p + 1 == pl.passes;
        const uint32_t left = precision - std::min(precision, 8 * (p + 1));
        CHECK(ps.slot == (p == 0 ? pl.pass0_slot : p) && ps.slot < (uint32_t)RADIX_MAX_PASSES);
        CHECK((ps.last != 0) == last);
        CHECK((ps.in == SORT_IN_DEPTH) == (p == 0));
        CHECK(!last || ps.out != SORT_OUT_PACKED);                                         // the last pass never packs
        CHECK(ps.out != SORT_OUT_PACKED || left + pl.val_bits <= 32);                      // a packing pass has room for what is left
        CHECK((ps.out == SORT_OUT_FINAL) == (last && p > 0));
        if (packed) CHECK(ps.in == SORT_IN_PACKED && ps.shift == 0 && ps.hist_shift == pl.val_bits);   // after a packing pass
        else CHECK(ps.in != SORT_IN_PACKED && ps.shift == 8 * p && ps.hist_shift == ps.shift);
        if (p > 0 && !packed) CHECK(ps.in == (pl.pass[p - 1].out == SORT_OUT_KV32 ? SORT_IN_KEYS32 : SORT_IN_KEYS16));
        CHECK(!ps.chunked || (pl.val_bits <= 24 && !in->sw.no_chunk && (ps.out == SORT_OUT_PACKED || ps.in == SORT_IN_PACKED)));   // chunked => val_bits <= 24
        CHECK(ps.grid >= 1 && ps.grid <= (uint32_t)(ps.chunked ? RADIX_MAX_BLOCKS : RADIX_TILE_GRID));
        CHECK(ps.grid == (ps.chunked ? radix_chunk_grid_for(pl.Rs) : radix_grid_for(pl.Rs)));
        CHECK((ps.skip_hist != 0) == (known && p == 0));                                   // skip_hist <=> known range, and only on pass 0
        CHECK((ps.in_narrow != 0) == (narrow && p == 0));
        CHECK(!ps.in_narrow || ps.out != SORT_OUT_KV32);
        CHECK(!ps.in_cull || (p == 0 && pl.cull));
        packed = packed || ps.out == SORT_OUT_PACKED;
    }
    for (uint32_t p = pl.passes; p < (uint32_t)RADIX_MAX_PASSES; p++) CHECK(pl.pass[p].grid == 0 && pl.pass[p].slot == 0);
    // the count is device-resident <=> cull, visibility cull or device-length list (and something is sorted)
    CHECK((pl.count_on_device != 0) == ((pl.cull || pl.vis_cull || in->count_on_device) && pl.Rs > 0));
    CHECK(pl.pass0_count <= SORT_COUNT_LIST && (pl.pass0_count == SORT_COUNT_HOST || pl.count_on_device));
    CHECK(!pl.pass0_publishes || pl.cull);
    *digest = *digest * 1099511628211ull + pl.front + 16 * pl.gather + 64 * pl.passes + 512 * pl.pass0_slot + 4096 * (uint64_t)pl.pass[0].grid +
              (1ull << 32) * pl.pass[0].out + (1ull << 36) * pl.pass[1].out + (1ull << 40) * pl.pass[0].chunked;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: sort_plan_fuzz <cases.bin | -> [random inputs] [seed]\n"); return 2; }
    const long randoms = argc > 2 ? atol(argv[2]) : 100000;
    const unsigned seed = argc > 3 ? (unsigned)atol(argv[3]) : 1u;
    uint64_t digest = 1469598103934665603ull;
    long from_file = 0;
    if (strcmp(argv[1], "-") != 0) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("%s: cannot be read\n", argv[1]); return 2; }
        SortPlanIn in;
        while (fread(&in, sizeof(in), 1, f) == 1) {
            run(in, &digest);
            from_file++;
        }
        fclose(f);
    }
    std::mt19937 rng(seed);
    auto u = [&](uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; };
    auto flag = [&]() { return u(4) == 0 ? 1u : 0u; };
    auto count = [&]() {                                   // small, around a tile / chunk boundary, around a power of two, anything
        switch (u(5)) {
        case 0: return u(4);
        case 1: return (1u + u(2048)) * 4096u + u(3) - 1u;
        case 2: return (1u << u(32)) + u(3) - 1u;
        case 3: return u(1u << 25);
        default: return (uint32_t)rng();
        }
    };
    long ranges = 0;
    for (long n = 0; n < randoms; n++) {
        SortPlanIn in = {};
        in.flags = u(6) == 0 ? u(8) : (u(3) ? GS_SORT_INTEGER : u(4));
        in.precision = u(8) == 0 ? u(41) : 8u + u(17);
        in.uploaded = count();
        in.sort_count = u(3) ? in.uploaded : count();
        in.render_count = u(3) ? in.uploaded : (u(2) ? in.sort_count : count());
        in.frustum_cull = flag(); in.visibility_cull = flag();
        in.clean_slot = u(8) == 0 ? rng() : (u(2) ? 3u : 0u);
        in.pending_gather = flag(); in.pending_keep_zeroed = flag();
        in.extreme_current = u(4) != 0; in.c16_current = u(2);
        in.list = u(3) ? SORT_LIST_IDENTITY : u(4);
        in.precomputed = u(5) ? SORT_PRE_NONE : u(4);
        in.count_on_device = u(8) == 0;
        in.mesh_map = flag(); in.mesh_uploaded = u(2) ? in.uploaded : count();
        in.mesh_strip = flag(); in.mesh_lazy_mask = flag();
        in.cu_count = u(16) == 0 ? 0u : 1u + u(1024);
        in.sw.tree_no_fuse = flag(); in.sw.vis_front = u(4) ? 0u : u(4); in.sw.no_pack = flag(); in.sw.no_chunk = flag();
        in.sw.no_known_range = u(8) == 0; in.sw.no_narrow_keys = flag(); in.sw.no_compact_centres = flag();
        // the range: of a random set under random coefficients, both branches of gs_key_range
        std::vector<int32_t> set((size_t)u(40) * 4);
        const uint32_t cbits = 1u + u(31), ibits = 1u + u(31);
        for (int32_t& v : set) v = (int32_t)((int64_t)(rng() >> (32u - cbits)) - ((int64_t)1 << (cbits - 1u)));
        int32_t im[3];
        for (int32_t& v : im) v = u(16) == 0 ? (u(2) ? INT32_MIN : INT32_MAX) : (int32_t)((int64_t)(rng() >> (32u - ibits)) - ((int64_t)1 << (ibits - 1u)));
        int32_t lo = 0, hi = 0;
        std::unique_ptr<int32_t[]> rows(new int32_t[set.size() ? set.size() : 1]);     // an exact-size block: a read past it is a report
        std::copy(set.begin(), set.end(), rows.get());
        in.range_ok = gs_key_range(set.empty() ? nullptr : rows.get(), set.size() / 4, im, &lo, &hi);
        CHECK(!in.range_ok || (!set.empty() && lo <= hi));
        if (in.range_ok) {
            ranges++;
            for (size_t r = 0; r < set.size() / 4; r++) {
                const __int128 v = (__int128)im[0] * set[4 * r] + (__int128)im[1] * set[4 * r + 1] + (__int128)im[2] * set[4 * r + 2];
                CHECK(v >= lo && v <= hi);
            }
        } else if (u(4) == 0) {
            in.range_ok = 1;                               // (the plan takes the caller's word: any range)
            lo = (int32_t)rng(); hi = (int32_t)rng();
        }
        in.range_lo = lo; in.range_hi = hi;
        run(in, &digest);
    }
    printf("sort_plan_fuzz: %ld case inputs, %ld random inputs (seed %u, %ld with an exact key range), digest %016llx, %d failed checks\n",
           from_file, randoms, seed, ranges, (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
