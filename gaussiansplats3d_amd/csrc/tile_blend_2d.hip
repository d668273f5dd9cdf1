// tile_blend_2d.hip — fragment stage + blend of a GS_MESH_SURFEL mesh (SplatRenderMode.TwoD): k_tile_blend's geometry - one
// 256-thread workgroup per 32x32-pixel bin, one wave64 per 16x16-pixel quadrant, four pixels per lane (x = lane & 15,
// y = (lane >> 4) + 4 g) - over the same entry lists.
//
// Restates the reference's 2D-Gaussian fragment shader and blend state
//   /root/reference/src/splatmesh/SplatMaterial2D.js:302-343   ray / splat intersection through vT, rho = min(rho3d, rho2d),
//                                                              depth < near_n discard, alpha = min(0.99, opa * exp(-rho / 2)),
//                                                              alpha < 1/255 discard (test_T never fires: alpha <= 0.99)
//   /root/reference/src/splatmesh/SplatMaterial2D.js:45-55     NormalBlending, depthTest, no depth write
// as the front-to-back composite C += T alpha rgb; T *= 1 - alpha over the bin's near -> far list, a quadrant retiring once all its
// pixels have T <= 1e-4 (tested after every 8th splat it composites, so the result is a function of its ordered survivors alone).
// A fragment exists where the rasteriser covers the pixel: its centre f = (x + 0.5, y + 0.5) - which is also the interpolated
// vFragCoord there - lies inside the quad the vertex stage left as a centre and an inverse 2x2 basis (SurfelRec).
//
// Built with -ffp-contract=off: every product and sum is rounded on its own, in the shader's stated order, so the per-fragment
// decisions (inside, p.z == 0, rho3d <= rho2d, depth < 0.2, alpha < 1/255) are those of tests/surfel_ref.py bit for bit but for exp.
//
// The parent list is scanned in batches of 256 entries, one per thread; an entry whose tile rect touches the bin is copied, record
// as it is (80 B), into LDS next to the 4-bit quadrant mask of its rect, and every wave walks its own survivors through
// wave-uniform 16-byte LDS reads.  No exact quadrant refinement, no deep pass, no chunk partials.
#include "blend_common.hpp"

constexpr uint32_t SURFEL_WORDS4 = sizeof(SurfelRec) / 16u;          // 5 x 16 bytes per staged surfel
// k_tile_blend's termination, rule and cadence taken over as they are (tile_blend.hip: Px::open, GS_BLEND_CHECK): a wave tests its
// quadrant after every 8th splat it composites and retires when no pixel has T > 1e-4.  Not tuned for surfels.
constexpr uint32_t SURFEL_CHECK = 8u;

template <bool DEPTH>
__global__ __launch_bounds__(BLEND_THREADS) void k_tile_blend_2d(FrameArgs fa, const uint4* __restrict__ recs2d, uint32_t bins) {
    __shared__ uint4 s_batch[BLEND_THREADS * SURFEL_WORDS4];           // 20 KiB
    __shared__ uint32_t s_qmask[BLEND_THREADS];
    __shared__ uint32_t s_live, s_walked[4];
    const uint32_t wg = blockIdx.x;
    if (wg >= bins) return;
    const uint32_t bin = fa.bin_order ? fa.bin_order[wg] : wg;         // scheduling only: every bin is drawn by exactly one workgroup
    const BinGeom bg(fa, bin);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t bx = bg.bx, by = bg.by, begin = bg.begin, n = bg.n;
    // this lane's four pixels: centres (absolute, exact in fp32), stored depths
    const uint32_t px = bx * GS_BIN + (wave & 1u) * GS_TILE + (lane & 15u);
    const uint32_t py0 = by * GS_BIN + (wave >> 1) * GS_TILE + (lane >> 4);
    const float fx = (float)px + 0.5f;
    float fy[4], dz[4], T[4], Cr[4], Cg[4], Cb[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const uint32_t py = py0 + 4u * g;
        fy[g] = (float)py + 0.5f;
        T[g] = 1.0f; Cr[g] = Cg[g] = Cb[g] = 0.0f;
        dz[g] = 1.2676506e30f;                                         // outside the frame / no destination depth: passes
        if (DEPTH && px < fa.width && py < fa.height) {
            dz[g] = fa.dst_depth[(size_t)py * fa.width + px];
            if (fa.depth_mode == 2u) dz[g] = (float)floor((double)dz[g] * 16777215.0 + 0.5);
        }
    }
    uint32_t walked = 0, scanned = 0, since_check = 0;
    bool live_wave = bg.live(fa, wave);

    for (uint32_t base = 0; base < n; base += BLEND_THREADS) {
        const uint32_t cnt = min((uint32_t)BLEND_THREADS, n - base);
        scanned += cnt;
        __syncthreads();                                               // the previous batch is consumed, s_live read by everyone
        uint32_t qm = 0;
        if (tid < cnt) {
            const uint32_t slot = fa.vals[begin + base + tid];
            qm = quadrant_mask(fa.rects[slot], bx, by);
            if (qm) {
                const uint4* src = recs2d + (size_t)slot * SURFEL_WORDS4;
#pragma unroll
                for (uint32_t k = 0; k < SURFEL_WORDS4 - 1u; k++) s_batch[tid * SURFEL_WORDS4 + k] = src[k];
                uint4 last = src[SURFEL_WORDS4 - 1u];                  // {i11, c0, c1, pad}: the pad word carries the window depth
                last.w = DEPTH ? __float_as_uint(fa.zrec[slot]) : 0u;
                s_batch[tid * SURFEL_WORDS4 + SURFEL_WORDS4 - 1u] = last;
            }
        }
        s_qmask[tid] = qm;
        if (tid == 0) s_live = 0u;
        __syncthreads();
        if (live_wave) {
            for (uint32_t g0 = 0; g0 < cnt && live_wave; g0 += 64) {
                unsigned long long m = __ballot((s_qmask[g0 + lane] >> wave) & 1u);     // this wave's survivors (wave-uniform)
                while (m) {
                    const uint32_t j = g0 + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    walked++;
                    const uint4* sp = &s_batch[j * SURFEL_WORDS4];
                    const uint4 w0 = sp[0], w1 = sp[1], w2 = sp[2], w3 = sp[3], w4 = sp[4];
                    const float tux = __uint_as_float(w0.x), tuy = __uint_as_float(w0.y), tuz = __uint_as_float(w0.z);
                    const float tvx = __uint_as_float(w0.w), tvy = __uint_as_float(w1.x), tvz = __uint_as_float(w1.y);
                    const float twx = __uint_as_float(w1.z), twy = __uint_as_float(w1.w), twz = __uint_as_float(w2.x);
                    const float qcx = __uint_as_float(w2.y), qcy = __uint_as_float(w2.z);
                    const float cx = __uint_as_float(w2.w), cy = __uint_as_float(w3.x);
                    const float i00 = __uint_as_float(w3.y), i01 = __uint_as_float(w3.z), i10 = __uint_as_float(w3.w), i11 = __uint_as_float(w4.x);
                    const float r = (float)(w4.y & 0xFFFFu) * (1.0f / 65535.0f), gch = (float)(w4.y >> 16) * (1.0f / 65535.0f);
                    const float b = (float)(w4.z & 0xFFFFu) * (1.0f / 65535.0f), opa = (float)(w4.z >> 16) * (1.0f / 65535.0f);
                    const float zs = __uint_as_float(w4.w);
                    // k = f.x * Tw - Tu: the same for the lane's four pixels
                    const float kx = fx * twx - tux, ky = fx * twy - tuy, kz = fx * twz - tuz;
                    const float dx = fx - cx, ddx = qcx - fx;
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const float dy = fy[g] - cy;
                        const float u = i00 * dx + i01 * dy, v = i10 * dx + i11 * dy;
                        bool keep = fabsf(u) <= 1.0f && fabsf(v) <= 1.0f;              // the rasteriser: pixel centre inside the quad
                        const float lx = fy[g] * twx - tvx, ly = fy[g] * twy - tvy, lz = fy[g] * twz - tvz;
                        const float p0 = ky * lz - kz * ly, p1 = kz * lx - kx * lz, p2 = kx * ly - ky * lx;   // cross(k, l)
                        keep = keep && p2 != 0.0f;
                        const float sx = p0 / p2, sy = p1 / p2;
                        const float rho3d = sx * sx + sy * sy;
                        const float ddy = qcy - fy[g];
                        const float rho2d = 2.0f * (ddx * ddx + ddy * ddy);
                        const float rho = rho3d < rho2d ? rho3d : rho2d;               // min(rho3d, rho2d)
                        const float depth = rho3d <= rho2d ? (sx * twx + sy * twy) + twz : twz;
                        keep = keep && !(depth < 0.2f);
                        const float power = -0.5f * rho;
                        keep = keep && !(power > 0.0f);
                        const float a0 = opa * expf(power);
                        const float alpha = a0 > 0.99f ? 0.99f : a0;                   // min(0.99, .)
                        keep = keep && alpha >= (1.0f / 255.0f);                       // (a NaN alpha draws nothing)
                        if (DEPTH) keep = keep && zs <= dz[g];
                        if (keep) {
                            const float w = T[g] * alpha;
                            Cr[g] = Cr[g] + w * r; Cg[g] = Cg[g] + w * gch; Cb[g] = Cb[g] + w * b;
                            T[g] = T[g] * (1.0f - alpha);
                        }
                    }
                    if (++since_check == SURFEL_CHECK) {
                        since_check = 0;
                        const float tmax = fmaxf(fmaxf(T[0], T[1]), fmaxf(T[2], T[3]));
                        if (__ballot(tmax > GS_T_EPS) == 0ull) {                       // the whole quadrant is saturated
                            live_wave = false;
                            break;
                        }
                    }
                }
            }
            if (live_wave) s_live = 1u;                                // (every lane stores the same word, as in k_tile_blend)
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane((int)s_live) == 0) break;   // every quadrant saturated or clipped: the rest of the list is hidden
    }
    // statistics in gs_launch_blend's layout: {entries scanned, 2 x pairs} per bin, and the (splat, quadrant) pairs walked
    if (lane == 0u) s_walked[wave] = walked;
    __syncthreads();
    if (tid == 0u) {
        const uint32_t pairs = s_walked[0] + s_walked[1] + s_walked[2] + s_walked[3];
        fa.bin_stats[bin] = make_uint2(scanned, 2u * pairs);
        fa.bin_pairs[bin] = pairs;
    }
    // rgb = C + T * dst.rgb, alpha = (1 - T) + T * dst.a: what NormalBlending, back to front, leaves (gs_mesh_set_destination)
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const uint32_t py = py0 + 4u * g;
        if (px < fa.width && py >= fa.y0 && py < fa.y1) {
            float a = 1.0f - T[g], cr = Cr[g], cg = Cg[g], cb = Cb[g];
            if (fa.dst_rgba) {
                const float4 d = unpack_rgba8(fa.dst_rgba[(size_t)py * fa.width + px]);
                cr = T[g] * d.x + cr; cg = T[g] * d.y + cg; cb = T[g] * d.z + cb; a = T[g] * d.w + a;
            }
            fa.out[(size_t)(py - fa.y0) * fa.width + px] = pack_rgba8(cr, cg, cb, a);
        }
    }
}

int gs_launch_blend_2d(gs_mesh* m, const ProjectParams& pp, uint8_t* out_dev) {
    const uint32_t bins = pp.bins_x * (pp.bin_row_end - pp.bin_row_begin);
    if (bins == 0) return GS_OK;
    GS_TRY(m->blend_stats.ensure((size_t)bins * 12));     // uint2 [bins] {scanned, halves} | uint32 [bins] pairs
    FrameArgs fa = frame_args(m, pp);
    fa.out = reinterpret_cast<uint32_t*>(out_dev);
    fa.bin_stats = m->blend_stats.as<uint2>();
    fa.bin_pairs = m->blend_stats.as<uint32_t>() + 2 * (size_t)bins;
    fa.bin_order = m->plan.order_taken ? m->blend_order.as<uint32_t>() : nullptr;
    const uint4* recs2d = m->set().recs2d.as<uint4>();
    if (fa.depth_mode) hipLaunchKernelGGL(k_tile_blend_2d<true>, dim3(bins), dim3(BLEND_THREADS), 0, m->ctx->stream, fa, recs2d, bins);
    else hipLaunchKernelGGL(k_tile_blend_2d<false>, dim3(bins), dim3(BLEND_THREADS), 0, m->ctx->stream, fa, recs2d, bins);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
