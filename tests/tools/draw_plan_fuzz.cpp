// tests/tools/draw_plan_fuzz.cpp — a stand-alone program over csrc/draw_plan.cpp (host only: nothing of HIP) for a sanitizer run by
// hand: the draw's host policy on the inputs of the test cases (`python tests/draw_plan_cases.py dump cases.bin`) and on seeded
// random inputs - zero counts, bins = 0, huge shifts, NaN and infinite matrix entries, every switch.  It checks what must hold for
// ANY input (no order without matching statistics, the deep pass's workgroups within what the device holds, ...) and prints one
// summary line; a sanitizer report or a failed check is what fails the run.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/draw_plan_fuzz.cpp gaussiansplats3d_amd/csrc/draw_plan.cpp -o draw_plan_fuzz && ./draw_plan_fuzz cases.bin 100000 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>

#include "draw_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 10) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// one input through the debug entry, and the five functions once more on their own; the input lives in an exact-size heap block
static void run(const gs_draw_plan_debug_in& src, uint64_t* digest) {
    std::unique_ptr<gs_draw_plan_debug_in> in(new gs_draw_plan_debug_in(src));
    std::unique_ptr<gs_draw_plan_debug_out> out(new gs_draw_plan_debug_out());
    CHECK(gs_debug_draw_plan(in.get(), out.get()) == 0);
    const uint32_t bins = in->bins_x * (in->bin_row_end - in->bin_row_begin);
    CHECK(out->blend_bins == bins);
    CHECK(!out->order_ok || (bins > 0 && bins <= 8192u && in->stats_bins == bins && !in->no_blend_order));
    CHECK(!out->order_wg || out->order_ok);
    CHECK(!out->order_taken || out->order_wg);
    CHECK(!out->deep_pass || (out->order_wg && in->draw_mode == GS_DRAW_FP32 && !in->no_deep && in->mirror[GS_MIRROR_DEEP_CANDIDATES] > 0));
    CHECK(abs(out->sx) <= 4096 && abs(out->sy) <= 4096);
    CHECK(out->unit_at <= bins);
    CHECK(out->deep_pass ? (out->unit_wgs >= 1 || in->cu_count * in->occupancy == 0) : out->unit_wgs == 0);
    CHECK(out->unit_wgs <= in->cu_count * in->occupancy);
    CHECK(out->list_shift == in->list_current || out->list_shift == GS_LIST_SHIFT_SMALL || out->list_shift == GS_LIST_SHIFT_LARGE ||
          out->list_shift == GS_LIST_SHIFT_BIG || out->list_shift == GS_LIST_SHIFT_HUGE);
    CHECK(out->block_test >= 0 && out->block_test <= 2 && (in->block_cull || out->block_test == 2));
    CHECK(out->room == in->need + in->need / 8 + 1024);
    CHECK(read_feedback(nullptr).deep_candidates == 0u && !read_feedback(nullptr).view_valid);
    *digest = *digest * 1099511628211ull + out->order_wg + 2 * out->order_taken + 4 * out->deep_pass + 8 * (uint32_t)out->block_test +
              32 * out->list_shift + 256 * (uint64_t)(uint32_t)out->sx + 65536 * (uint64_t)out->unit_wgs;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: draw_plan_fuzz <cases.bin | -> [random inputs] [seed]\n"); return 2; }
    const long randoms = argc > 2 ? atol(argv[2]) : 100000;
    const unsigned seed = argc > 3 ? (unsigned)atol(argv[3]) : 1u;
    uint64_t digest = 1469598103934665603ull;
    long from_file = 0;
    gs_draw_plan_debug_in base;
    memset(&base, 0, sizeof(base));
    bool have_base = false;
    if (strcmp(argv[1], "-") != 0) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("%s: cannot be read\n", argv[1]); return 2; }
        gs_draw_plan_debug_in in;
        while (fread(&in, sizeof(in), 1, f) == 1) {
            if (!have_base) { base = in; have_base = true; }
            run(in, &digest);
            from_file++;
        }
        fclose(f);
    }
    std::mt19937 rng(seed);
    auto u = [&](uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; };
    auto flag = [&]() { return u(4) == 0 ? 1u : 0u; };
    const float odd[] = {0.0f, -0.0f, NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 1e-30f, 1.0f, -1.0f, 3.0e38f};
    auto matrix = [&](float* m, const float* like) {
        for (int k = 0; k < 16; k++) {
            const uint32_t pick = u(10);
            if (pick < 6 && like) m[k] = like[k];                                   // mostly a real camera, damaged in places
            else if (pick < 8) m[k] = (float)((double)rng() / 4294967296.0 * 20.0 - 10.0);
            else m[k] = odd[u(sizeof(odd) / sizeof(odd[0]))];
        }
    };
    for (long n = 0; n < randoms; n++) {
        gs_draw_plan_debug_in in = base;
        for (int k = 0; k < 3; k++) in.centre_sum[k] = u(8) == 0 ? (double)odd[u(11)] : ((double)rng() / 4294967296.0 - 0.5) * 1e4;
        in.centre_n = u(6) == 0 ? 0u : (u(6) == 0 ? ~0ull : 1u + u(100000));
        for (uint32_t k = 0; k < GS_MIRROR_WORDS; k++) in.mirror[k] = u(3) == 0 ? 0u : (u(3) == 0 ? ~0u : u(2048));
        in.tiles16 = u(8) == 0 ? ~0ull : (uint64_t)rng() * (u(4) == 0 ? rng() : 1u);
        in.need = u(8) == 0 ? ~0ull - u(4096) : (uint64_t)rng() << u(33);
        in.visible = u(5) == 0 ? 0u : rng();
        in.list_current = u(8);
        matrix(in.stats_view, have_base ? base.stats_view : nullptr);
        matrix(in.stats_proj, have_base ? base.stats_proj : nullptr);
        if (u(3)) memcpy(in.proj, in.stats_proj, sizeof(in.proj)); else matrix(in.proj, have_base ? base.proj : nullptr);
        if (u(4) == 0) memcpy(in.view, in.stats_view, sizeof(in.view)); else matrix(in.view, have_base ? base.view : nullptr);
        in.width = in.stats_width = (float)(1u + u(65536));
        in.height = in.stats_height = (float)(u(16) == 0 ? 0u : 1u + u(65536));
        if (u(8) == 0) in.stats_width = (float)(1u + u(65536));
        in.count = in.stats_count = u(4) == 0 ? 0u : rng();
        in.list_shift = in.stats_list_shift = 1u + u(5);
        if (u(8) == 0) in.stats_list_shift = 1u + u(5);
        in.bins_x = u(8) == 0 ? 0u : 1u + u(300);
        in.bin_row_begin = u(4) ? 0u : u(200);
        in.bin_row_end = u(8) == 0 ? in.bin_row_begin : in.bin_row_begin + u(140);   // (equal: bins = 0)
        const uint32_t bins = in.bins_x * (in.bin_row_end - in.bin_row_begin);
        in.stats_valid = u(8) ? 1u : 0u;
        in.stats_bins = u(6) ? bins : rng();
        in.stats_row_begin = u(6) ? in.bin_row_begin : u(200);
        in.stats_width_px = u(6) ? (uint32_t)in.width : u(65536);
        in.draw_mode = u(4) ? GS_DRAW_FP32 : u(3);
        in.stats_mode = u(6) ? in.draw_mode : u(3);
        in.block_cull = u(6) ? 1u : 0u;
        in.draw_serial = u(4) ? u(64) : rng();
        in.no_deep = flag();
        in.deep_min = u(4) ? 4096u : rng();
        in.deep_factor = u(4) ? 3u : rng();
        in.no_blend_order = u(8) == 0;
        in.order_motion = u(3) == 0 ? odd[u(11)] : (u(2) ? 0.045f : (float)u(100) * 0.01f);
        in.no_stat_shift = flag(); in.blend_order_stale = flag(); in.deep_row_major_on_motion = flag(); in.deep_units_last = flag();
        in.cu_count = u(8) == 0 ? 0u : 1u + u(1024);
        in.occupancy = u(8) == 0 ? 0u : 1u + u(16);
        in.measured_count = u(4) == 0 ? 0u : rng();
        in.measured_visible = u(4) == 0 ? 0u : (u(2) ? rng() : u(in.measured_count + 1u));
        in.strip = flag(); in.no_block_list = flag(); in.block_test_always = flag();
        run(in, &digest);
    }
    printf("draw_plan_fuzz: %ld case inputs, %ld random inputs (seed %u), digest %016llx, %d failed checks\n", from_file, randoms, seed,
           (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
