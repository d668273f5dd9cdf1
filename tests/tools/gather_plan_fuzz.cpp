// tests/tools/gather_plan_fuzz.cpp — a stand-alone program over csrc/gather_plan.cpp (host only: nothing of HIP) for a sanitizer
// run by hand: the gather's host policy on the inputs of the test cases (`python tests/gather_plan_cases.py dump cases.bin`) and
// on seeded random inputs - scene counts 0 .. 40, empty scenes, zero, huge, denormal and non-finite boxes and matrices, fov and
// render sizes of any sign - and the hand-over's transitions on seeded random scripts of events, replayed in exact-size heap
// blocks.  It checks what must hold for ANY input and prints one summary line; a sanitizer report or a failed check is what
// fails the run.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I gaussiansplats3d_amd/csrc \
//       tests/tools/gather_plan_fuzz.cpp gaussiansplats3d_amd/csrc/gather_plan.cpp -o gather_plan_fuzz && ./gather_plan_fuzz cases.bin 100000 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>

#include "gather_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 10) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// one input through the debug entry; the input and the plan live in exact-size heap blocks
static void run(const GatherPlanIn& src, uint64_t* digest) {
    std::unique_ptr<GatherPlanIn> in(new GatherPlanIn(src));
    std::unique_ptr<GatherPlan> out(new GatherPlan());
    CHECK(gs_debug_gather_plan(in.get(), out.get()) == 0);
    const GatherPlan& pl = *out;
    CHECK(pl.scale > 0.0);                                  // never NaN, zero or negative whatever came in (tree_bucket clamps the rest)
    CHECK(pl.deferred <= 1u && pl.zero_keep <= 1u && pl.scene_table <= 1u);
    CHECK(!pl.zero_keep || (pl.deferred && in->frustum_cull));
    CHECK(!pl.deferred || (in->leaves && in->has_sorter && !in->host_copy && !(in->sorter_flags & GS_SORT_DYNAMIC) && !in->no_defer && !pl.scene_table));
    CHECK(pl.scene_table == (in->scene_count > 1u));
    CHECK(pl.keep_words == (pl.zero_keep ? (uint32_t)(((uint64_t)in->tree_splats + 63) / 64 + 2) : 0u));
    // the zeroed prefix lies inside the keep mask of any sorter gs_tree_gather accepts (max_count >= the tree's splats)
    CHECK(!pl.zero_keep || in->max_count < in->tree_splats || (size_t)pl.keep_words * 8 <= sorter_keep_mask_bytes(in->max_count));
    CHECK((uint64_t)pl.leaf_grid * PLAN_THREADS >= in->leaves && (uint64_t)pl.leaf_grid * PLAN_THREADS < (uint64_t)in->leaves + PLAN_THREADS);
    uint64_t s;
    memcpy(&s, &pl.scale, 8);
    *digest = *digest * 1099511628211ull + s + pl.deferred + 2 * pl.zero_keep + 4 * pl.scene_table + 8 * (uint64_t)pl.leaf_grid;
}

// a random script of events through the replay entry, checked for the invariant after every step
static void replay(std::mt19937& rng, uint32_t n, uint64_t* digest) {
    auto u = [&](uint32_t m) { return (uint32_t)(rng() % m); };
    std::unique_ptr<gs_handover_event[]> ev(new gs_handover_event[n]);
    std::unique_ptr<gs_handover_step[]> st(new gs_handover_step[n]);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t kind = u(HANDOVER_EV_KINDS);
        ev[k] = {kind, u(2), u(kind == HANDOVER_EV_GATHER ? 3u : 2u), u(2) ? u(2) : (uint32_t)rng(), u(2), u(2) ? u(3) : (uint32_t)rng(), u(2)};
    }
    CHECK(gs_debug_gather_handover(ev.get(), n, st.get()) == 0);
    for (uint32_t k = 0; k < n; k++) {
        const gs_handover_step& o = st[k];
        for (uint32_t t = 0; t < 2u; t++)
            for (uint32_t s = 0; s < 2u; s++) CHECK((o.planner[t] == s) == (o.state[s] == HANDOVER_PLANNED && o.tree_of[s] == t));
        for (uint32_t s = 0; s < 2u; s++) {
            CHECK(o.state[s] <= HANDOVER_COPIED);
            CHECK(o.state[s] == HANDOVER_PLANNED || (o.tree_of[s] == 2u && !o.keep_zeroed[s]));
            CHECK(o.state[s] != HANDOVER_NONE || (o.count[s] == 0u && !o.count_on_device[s]));
        }
        CHECK(o.evicted == 2u || (ev[k].kind == HANDOVER_EV_GATHER && o.evicted != ev[k].sorter && o.state[o.evicted] == HANDOVER_COPIED));
        CHECK(o.refused <= HANDOVER_SORT_PARTIAL_ASYNC && o.sort_count <= o.render_count);
        *digest = *digest * 1099511628211ull + o.state[0] + 4 * o.state[1] + 16 * o.planner[0] + 64 * o.planner[1] + 256 * o.evicted + 1024 * o.refused;
    }
    gs_handover_event bad = {HANDOVER_EV_KINDS, 0, 0, 0, 0, 0, 0};
    CHECK(gs_debug_gather_handover(&bad, 1, st.get()) == -1);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: gather_plan_fuzz <cases.bin | -> [random inputs] [seed]\n"); return 2; }
    const long randoms = argc > 2 ? atol(argv[2]) : 100000;
    const unsigned seed = argc > 3 ? (unsigned)atol(argv[3]) : 1u;
    uint64_t digest = 1469598103934665603ull;
    long from_file = 0;
    if (strcmp(argv[1], "-") != 0) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("%s: cannot be read\n", argv[1]); return 2; }
        std::unique_ptr<GatherPlanIn> in(new GatherPlanIn());
        while (fread(in.get(), sizeof(GatherPlanIn), 1, f) == 1) {
            run(*in, &digest);
            from_file++;
        }
        fclose(f);
    }
    std::mt19937 rng(seed);
    auto u = [&](uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; };
    auto flag = [&]() { return u(3) == 0 ? 1u : 0u; };
    auto real = [&]() -> double {                          // ordinary, tiny, huge, zero, non-finite, any bit pattern
        const double x = ((double)rng() / 4294967296.0 - 0.5) * 2.0;
        switch (u(12)) {
        case 0: return 0.0;
        case 1: return x * 1e-310;
        case 2: return x * 1e300;
        case 3: return u(2) ? INFINITY : -INFINITY;
        case 4: return NAN;
        case 5: { uint64_t b = ((uint64_t)rng() << 32) | rng(); double d; memcpy(&d, &b, 8); return d; }
        case 6: return x * 1e6;
        default: return x * 20.0;
        }
    };
    std::unique_ptr<GatherPlanIn> in(new GatherPlanIn());
    for (long n = 0; n < randoms; n++) {
        memset(in.get(), 0, sizeof(GatherPlanIn));
        for (double& v : in->model_view) v = real();
        in->fov_y_deg = u(4) ? 5.0 + u(166) : real();
        in->render_width = u(4) ? 1.0 + u(8000) : real();
        in->render_height = u(4) ? 1.0 + u(8000) : real();
        in->gather_all = flag();
        in->leaves = u(4) ? u(100000) : rng();
        in->tree_splats = u(4) ? u(1u << 24) : rng();
        in->scene_count = u(8) ? 1u + u(GS_MAX_SCENES) : u(41);
        in->has_sorter = u(2); in->sorter_flags = u(4); in->frustum_cull = flag();
        in->max_count = u(2) ? in->tree_splats + u(1000) : rng();
        in->host_copy = flag(); in->count_on_device = flag(); in->no_defer = flag();
        for (uint32_t s = 0; s < GS_MAX_SCENES; s++) {
            GatherScene& sc = in->scene[s];
            for (double& v : sc.box) v = real();
            for (double& v : sc.model_view) v = u(3) ? in->model_view[&v - sc.model_view] : real();
            sc.empty = flag();
        }
        run(*in, &digest);
    }
    const long scripts = randoms / 100 + 1;
    for (long n = 0; n < scripts; n++) replay(rng, 1u + u(200), &digest);
    printf("gather_plan_fuzz: %ld case inputs, %ld random inputs, %ld random hand-over scripts (seed %u), digest %016llx, %d failed checks\n",
           from_file, randoms, scripts, seed, (unsigned long long)digest, failures);
    return failures ? 1 : 0;
}
