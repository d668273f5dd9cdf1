// blend_common.hpp — what the blend kernels of tile_blend.hip (3D splats) and tile_blend_2d.hip (surfels) share: the launch
// geometry, a draw's lists and frame as a kernel argument, the rect -> quadrant mask and the RGBA8 conversions.  Text moved out of
// tile_blend.hip unchanged.
#pragma once
#include "gs_internal.hpp"

constexpr float GS_T_EPS = 1e-4f;
constexpr int BLEND_THREADS = 256;

// which of the 2x2 tiles of the 32-px bin (bx, by) the splat's 16-px tile rect touches: bit (qx + 2*qy).  The rect is the
// vertex stage's own (k_project), so the blend takes exactly its per-tile decisions (a strip of a multi-GPU draw then
// reproduces the full frame bit for bit).
__device__ __forceinline__ uint32_t quadrant_mask(uint2 r16, uint32_t bx, uint32_t by) {
    const uint32_t x0 = r16.x & 0xFFFFu, y0 = r16.x >> 16, x1 = r16.y & 0xFFFFu, y1 = r16.y >> 16;
    const uint32_t cx = 2u * bx, cy = 2u * by;
    const uint32_t mx = ((cx >= x0 && cx <= x1) ? 1u : 0u) | ((cx + 1u >= x0 && cx + 1u <= x1) ? 2u : 0u);
    const uint32_t my = ((cy >= y0 && cy <= y1) ? 1u : 0u) | ((cy + 1u >= y0 && cy + 1u <= y1) ? 2u : 0u);
    return (mx & (my & 1u ? 3u : 0u)) | ((mx & (my & 2u ? 3u : 0u)) << 2);
}

struct FrameArgs {
    const uint2* __restrict__ ranges;
    const uint32_t* __restrict__ vals;
    const uint4* __restrict__ recs;
    const uint2* __restrict__ rects;
    uint32_t* __restrict__ out;
    uint32_t width, y0, y1, bins_x, bin_row_begin, lists_x, list_row_begin, list_shift;
    uint2* __restrict__ bin_stats;
    uint32_t* __restrict__ bin_pairs;
    const uint32_t* __restrict__ bin_order;
    // destination (gs_mesh_set_destination): the splats' window depths (per record slot), the stored depth and colour of the whole
    // frame (row 0 = bottom, `width` pixels per row), and how depths compare (1 = fp32, 2 = both sides as 24-bit integers)
    const float* __restrict__ zrec;
    const float* __restrict__ dst_depth;
    const uint32_t* __restrict__ dst_rgba;
    uint32_t depth_mode, height;
};

struct BinGeom {
    uint32_t bx, by, begin, n;
    __device__ __forceinline__ BinGeom(const FrameArgs& fa, uint32_t bin) {
        bx = bin % fa.bins_x; by = bin / fa.bins_x + fa.bin_row_begin;
        const uint32_t per_list = fa.list_shift - GS_BIN_SHIFT;      // the entry list of the list bin this 32-px bin lies in
        const uint32_t list_id = ((by >> per_list) - fa.list_row_begin) * fa.lists_x + (bx >> per_list);
        const uint2 range = fa.ranges[list_id];
        begin = range.x; n = range.y > range.x ? range.y - range.x : 0u;   // untouched bins keep (~0, 0)
    }
    // a quadrant outside the viewport / this rank's strip of pixel rows has nothing to draw
    __device__ __forceinline__ bool live(const FrameArgs& fa, uint32_t q) const {
        const uint32_t qx0 = bx * GS_BIN + (q & 1u) * GS_TILE, qy0 = by * GS_BIN + (q >> 1) * GS_TILE;
        return qx0 < fa.width && qy0 < fa.y1 && qy0 + GS_TILE > fa.y0;
    }
};

// an RGBA8 word (r in the low byte) as channel values k / 255
__device__ __forceinline__ float4 unpack_rgba8(uint32_t d) {
    return make_float4((float)(d & 255u) * (1.0f / 255.0f), (float)((d >> 8) & 255u) * (1.0f / 255.0f),
                       (float)((d >> 16) & 255u) * (1.0f / 255.0f), (float)(d >> 24) * (1.0f / 255.0f));
}
// ... and back, as the draws round a frame: clamp, then x 255 + 0.5 as ONE fma (no pragma here: both callers always contracted it).
// k_rop8_window keeps the oracle's unfused mul, add under its own pragma, so it does not share this.
__device__ __forceinline__ uint32_t pack_rgba8(float r, float g, float b, float a) {
    auto u8 = [](float v) { return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); };
    return u8(r) | (u8(g) << 8) | (u8(b) << 16) | (u8(a) << 24);
}

// what every kernel here reads of a draw: the lists and records of the last binning, the frame's and the strip's geometry, and the
// destination as the kernels see it (pp.depth_mode was derived from the same fields: mesh_params)
static FrameArgs frame_args(const gs_mesh* m, const ProjectParams& pp) {
    FrameArgs fa = {};
    const ProjSet& ps = m->set();                          // the set the draw was binned from
    fa.ranges = m->tile_ranges.as<uint2>();
    fa.vals = (m->sorted_buf ? m->evalB : m->evalA).as<uint32_t>();
    fa.recs = ps.recs.as<uint4>();
    fa.rects = ps.rects.as<uint2>();
    fa.width = (uint32_t)pp.width; fa.height = (uint32_t)pp.height; fa.y0 = pp.y0; fa.y1 = pp.y1;
    fa.bins_x = pp.bins_x; fa.bin_row_begin = pp.bin_row_begin;
    // (list_shift counts 16-px tiles per list bin edge, as in the binner: a list bin is (16 << list_shift) px)
    fa.lists_x = pp.lists_x; fa.list_row_begin = pp.list_row_begin; fa.list_shift = pp.list_shift;
    fa.depth_mode = pp.depth_mode;
    fa.zrec = pp.depth_mode ? ps.zrec.as<float>() : nullptr;
    fa.dst_depth = pp.depth_mode ? m->dest_depth : nullptr;
    fa.dst_rgba = m->dest_rgba;
    return fa;
}
