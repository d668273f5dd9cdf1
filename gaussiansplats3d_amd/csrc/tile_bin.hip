// tile_bin.hip — order-preserving duplication of splats into the entry lists of the screen's list bins.
//
// The reference has no binning: it draws one instanced quad per splat, back to front, and lets the ROPs blend
// (/root/reference/src/splatmesh/SplatGeometry.js:11-37, SplatMaterial3D.js:65-75, src/Viewer.js:1616).  A
// tile rasteriser needs each tile's splats as a list in that same draw order, so:
//   k_bin_count   walk the sorted index list NEAR->FAR (q = R-1-p).  One flag per 256-splat storage block (block_any, kept as a
//                 bitmap in LDS) filters the list before anything is gathered; a position of a live block gathers ONE word
//                 written by k_project - {visible, record slot in the block, tile rect}, 4 bytes on frames of <= 256 x 256
//                 tiles and 8 beyond (bin_word.hpp); the few rects the 4-byte word cannot hold (a span over 14 tiles: 0.36 %
//                 of C3's visible splats) cost their lanes a second, dependent gather of the record's own rect.  Survivors are
//                 compacted (wave64 ballot + popcount prefix) into the workgroup's own slice of a (slot, rect, offset) list,
//                 and entry counts are reduced.  The kernel is a chain of random gathers, and what they cost follows the
//                 words' footprint in the live blocks (profiles/r12_gather_live_blocks.txt).
//   k_bin_emit    splat-centric expansion into (list bin, record slot) pairs, one lane per surviving splat, runs
//                 written at the offsets the count pass fixed; each workgroup scans the binning workgroups' counts itself
//                 (no scan kernel) and takes batches of 256 splats round-robin, so the near end of the list - whose splats
//                 touch 30x the mean number of lists - is spread over the whole grid.  Only batches that hold a splat are
//                 dealt (draw_plan.hpp: live units), and a workgroup loads its next batch before it expands this one.
//   entry sort    stable LSD radix passes on the list-bin id (radix.hpp): stability keeps near->far order per list;
//                 one pass for <= 256 lists (1080p at 128-px lists), and the pass publishes every list's [begin,end)
// Entry count D only ever lives on the device; downstream grids are sized for the capacity and read D there.
#include <stdlib.h>

#include "radix.hpp"

constexpr int BIN_THREADS = 256;
#ifndef BIN_PER_LANE
#define BIN_PER_LANE 4
#endif
#ifndef BIN_MAX_BLOCKS_CFG
#define BIN_MAX_BLOCKS_CFG 2048
#endif
constexpr int BIN_MAX_BLOCKS = BIN_MAX_BLOCKS_CFG;        // 8 workgroups of 256 per CU: full wave occupancy
constexpr uint32_t ANY_WORDS = 2048;                      // coarse visibility bits kept in LDS: 65536 blocks = 16.7 M splats

// vertex-stage rects are in 16-px tiles; the entry lists are per list bin of (16 << list_shift) px
__device__ __forceinline__ uint32_t rect_tiles(uint2 r) {
    const uint32_t x0 = r.x & 0xFFFFu, y0 = r.x >> 16, x1 = r.y & 0xFFFFu, y1 = r.y >> 16;
    return (x1 >= x0 && y1 >= y0) ? (x1 - x0 + 1u) * (y1 - y0 + 1u) : 0u;
}
// 16-px tile rect -> list-bin rect: per-field shift of (x | y << 16) with the bits that cross the field boundary masked
__device__ __forceinline__ uint2 rect_to_bins(uint2 r, uint32_t list_shift) {
    const uint32_t field = 0xFFFFu >> list_shift, mask = field | (field << 16);
    return make_uint2((r.x >> list_shift) & mask, (r.y >> list_shift) & mask);
}

struct BinChunk {
    uint32_t begin, end;   // batch indices (256 list positions per batch)
    uint32_t id;           // chunk index: workgroups of one XCD walk neighbouring chunks of the sorted list (radix.hpp, xcd_chunk)
};
__device__ __forceinline__ BinChunk bin_chunk(uint32_t n) {
    const uint32_t batches = (n + BIN_THREADS - 1) / BIN_THREADS;
    const uint32_t per = (batches + gridDim.x - 1) / gridDim.x;
    BinChunk c;
    c.id = xcd_chunk(blockIdx.x, gridDim.x);
    c.begin = min(c.id * per, batches);
    c.end = min(c.begin + per, batches);
    return c;
}

// block_sums layout: [0,BIN_MAX_BLOCKS) entries per workgroup | [BIN_MAX_BLOCKS, 2*BIN_MAX_BLOCKS) compacted (visible) splats per
// workgroup | [2*BIN_MAX_BLOCKS, 3*BIN_MAX_BLOCKS) 16-px tiles touched (statistics)
// Each lane owns 4 consecutive list positions per iteration, so 4 index loads, then 4 mask look-ups, then up to 4
// rect gathers are in flight together (the kernel is a chain of dependent memory round trips), and one packed
// 64-bit block scan per 1024 positions yields both the compaction slot and the entry offset.
#ifdef GS_BIN_PROFILE
// tools/bin_profile.py: per workgroup of k_bin_count [0] / k_bin_emit [1]: {start, after the prologue, end} of the 100 MHz
// clock and the workgroup's output count (k_bin_emit: | the live units it expanded << 32)
__device__ unsigned long long g_bin_prof[2 * 2048 * 4];
extern "C" int gs_debug_bin_prof(void* dst) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_bin_prof), sizeof(unsigned long long) * 2 * 2048 * 4, 0, hipMemcpyDeviceToHost);
}
#define BIN_PROF(k, slot, v) do { if (threadIdx.x == 0 && blockIdx.x < 2048u) g_bin_prof[((k) * 2048 + blockIdx.x) * 4 + (slot)] = (v); } while (0)
#else
#define BIN_PROF(k, slot, v) do { } while (0)
#endif

// The count pass over one workgroup's slice [pos_begin, pos_end) of the near->far walk: filter, one gather per position of a live
// block, compaction into the slice of (slot, rect, first entry) lists (k_bin_count).
struct SliceCount {
    uint32_t entries, splats, t16;       // entries emitted by the slice | compacted (visible) splats | this LANE's 16-px tiles (statistics)
};
// NARROW: prect holds the 4-byte word; `rects` (the record set's per-slot rects) answers its escapes.
template <bool NARROW>
__device__ __forceinline__ SliceCount bin_count_slice(const uint32_t* __restrict__ order, uint32_t R, const uint32_t* __restrict__ perm,
                                                      const void* __restrict__ prect, const uint2* __restrict__ rects,
                                                      uint32_t* __restrict__ cidx, uint2* __restrict__ crect,
                                                      uint32_t* __restrict__ coff, uint32_t list_shift, uint32_t splat_count,
                                                      const uint8_t* __restrict__ block_any, bool coarse, const uint32_t* s_any,
                                                      unsigned long long* s_w, uint32_t pos_begin, uint32_t pos_end) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t sum = 0;                                      // entries emitted so far by this workgroup
    uint32_t out = pos_begin;                              // next slot of this workgroup's compacted slice
    uint32_t t16 = 0;                                      // 16-px tiles touched by this lane's splats (statistics only)
    for (uint32_t pos0 = pos_begin; pos0 < pos_end; pos0 += BIN_PER_LANE * BIN_THREADS) {
        const uint32_t q0 = pos0 + (uint32_t)BIN_PER_LANE * threadIdx.x;
        uint32_t idx[BIN_PER_LANE];
        bool keep[BIN_PER_LANE];
        uint2 r[BIN_PER_LANE];
#pragma unroll
        for (int k = 0; k < BIN_PER_LANE; k++) {
            const uint32_t q = q0 + k;
            keep[k] = q < pos_end;
            const uint32_t p = R - 1u - min(q, R - 1u);    // draw order is back-to-front; we go front-to-back
            idx[k] = order ? order[p] : p;
            // a stale or wrong caller list must not fault the GPU (WebGL's texelFetch out of range is harmless too):
            // entries beyond the uploaded splats draw nothing
            keep[k] = keep[k] && idx[k] < splat_count;
            idx[k] = min(idx[k], splat_count - 1u);
        }
        if (perm) {                                        // caller's splat index -> internal (Morton) position
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) idx[k] = perm[idx[k]];
        }
        // k_project compacts survivors inside their 256-splat block and leaves, per position of a live block, one word
        // {visible, slot in the block, tile rect} (bin_word.hpp): a single gather gives the filter, the slot and the rect
        if (coarse) {
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) keep[k] = keep[k] && ((s_any[idx[k] >> 13] >> ((idx[k] >> 8) & 31u)) & 1u);
        } else if (block_any) {                            // more blocks than the LDS bitmap holds: the flag byte itself
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) keep[k] = keep[k] && block_any[idx[k] >> 8] != 0;
        }
        uint32_t slot[BIN_PER_LANE];
        if (NARROW) {
            uint32_t w[BIN_PER_LANE];
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) w[k] = keep[k] ? static_cast<const uint32_t*>(prect)[idx[k]] : BIN_WORD_INVISIBLE;
            bool esc[BIN_PER_LANE];
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) {
                const BinWordOut o = bin_word_unpack_narrow(w[k]);
                keep[k] = o.visible;                       // (a position that was not kept carries the invisible word)
                esc[k] = o.escape;
                slot[k] = (idx[k] & ~255u) + o.slot;
                r[k] = make_uint2(o.rect.lo, o.rect.hi);
            }
            // a rect the word could not hold: the record's own, one more dependent gather for these few lanes
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++)
                if (esc[k]) r[k] = rects[slot[k]];
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++)
                if (!keep[k]) r[k] = make_uint2(0xFFFFu, 0u);
        } else {
#pragma unroll
            for (int k = 0; k < BIN_PER_LANE; k++) {
                const uint2 g = keep[k] ? static_cast<const uint2*>(prect)[idx[k]] : make_uint2(0u, 0u);
                const BinWordOut o = bin_word_unpack_wide(BinWordWide{g.x, g.y});
                keep[k] = keep[k] && o.visible;
                slot[k] = (idx[k] & ~255u) + o.slot;
                r[k] = keep[k] ? make_uint2(o.rect.lo, o.rect.hi) : make_uint2(0xFFFFu, 0u);
            }
        }
#pragma unroll
        for (int k = 0; k < BIN_PER_LANE; k++) t16 += rect_tiles(r[k]);
        uint32_t n[BIN_PER_LANE], cnt = 0, ent = 0;
#pragma unroll
        for (int k = 0; k < BIN_PER_LANE; k++) {
            n[k] = keep[k] ? rect_tiles(rect_to_bins(r[k], list_shift)) : 0u;   // entries = list bins touched
            cnt += keep[k] ? 1u : 0u;
            ent += n[k];
        }
        // packed inclusive scan: high word = compacted splats, low word = tile entries (both < 2^31 per workgroup)
        const unsigned long long mine = ((unsigned long long)cnt << 32) | ent;
        const unsigned long long incl = wave_incl_scan(mine, lane);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        unsigned long long base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const unsigned long long c = s_w[w];
            base += ((uint32_t)w < wave) ? c : 0ull;
            total += c;
        }
        const unsigned long long excl = base + incl - mine;
        uint32_t o = out + (uint32_t)(excl >> 32);
        uint32_t e = sum + (uint32_t)excl;
#pragma unroll
        for (int k = 0; k < BIN_PER_LANE; k++) {
            if (keep[k]) {
                cidx[o] = slot[k];                         // what the blend gathers records by
                crect[o] = r[k];
                coff[o] = e;                               // first entry slot of this splat, relative to the workgroup
                o++;
                e += n[k];
            }
        }
        out += (uint32_t)(total >> 32);
        sum += (uint32_t)total;
        __syncthreads();
    }
    SliceCount sc;
    sc.entries = sum; sc.splats = out - pos_begin; sc.t16 = t16;
    return sc;
}

// (waves_per_eu 8: at 62 VGPRs the compiler reports 8 waves per SIMD, yet only 7 workgroups per CU became resident and the last
// 256 of the 2048 started 10 us late - r02v timeline; with the attribute all start together: span 35.4 -> 33.0 us.
// Dealing spans of 1024 positions round-robin instead of one contiguous chunk per workgroup, with a scan kernel between count
// and emit, was tried as well: the entries per workgroup even out (max 1841 vs 3681) but the body time does not - 24.6 us max
// either way, it is a chain of loaded memory round trips - and the extra kernel makes the C3 frame 3 us slower.)
template <bool NARROW>
__global__ __launch_bounds__(BIN_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_bin_count(const uint32_t* __restrict__ order, uint32_t R_host,
                                                           const uint32_t* __restrict__ R_dev /* nullable */,
                                                           const uint32_t* __restrict__ perm,
                                                           const void* __restrict__ prect,
                                                           const uint2* __restrict__ rects /* the same set's: a narrow word's escapes */,
                                                           uint32_t* __restrict__ cidx,
                                                           uint2* __restrict__ crect, uint32_t* __restrict__ coff,
                                                           uint32_t* __restrict__ block_sums,
                                                           uint32_t* __restrict__ digit_total,
                                                           uint2* __restrict__ tile_ranges, uint32_t tiles, uint32_t list_shift,
                                                           uint32_t splat_count, const uint8_t* __restrict__ block_any,
                                                           uint32_t* __restrict__ deep_flags, uint32_t blend_bins,
                                                           uint32_t lds_bitmap /* 0: $GSPLAT_NO_COARSE_VIS, the flag bytes themselves */) {
    __shared__ unsigned long long s_w[4];
    // Coarse visibility, one bit per 256-splat storage block, in LDS.  75 % of a scene's splats draw nothing and, stored along
    // a Morton curve, mostly whole blocks of them; an LDS bit test spares those list positions the L2 gather of their
    // visibility word (5.8 M random L2 transactions per frame were this kernel's real cost: making the rects dense did nothing)
    __shared__ uint32_t s_any[ANY_WORDS];
    BIN_PROF(0, 0, wall_clock64());
    const uint32_t blocks = (splat_count + 255u) >> 8;
    const bool coarse = block_any != nullptr && blocks <= ANY_WORDS * 32u && lds_bitmap != 0u;
    if (coarse) {
        for (uint32_t w = threadIdx.x; w < (blocks + 31u) / 32u; w += BIN_THREADS) {
            const uint4* src = reinterpret_cast<const uint4*>(block_any + 32u * w);      // the buffer is padded to 64 bytes
            const uint4 a = src[0], b = src[1];
            const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 8; k++)                                                   // 4 flag bytes per word -> 4 bits
                bits |= (((v[k] & 0xFFu) ? 1u : 0u) | ((v[k] & 0xFF00u) ? 2u : 0u) | ((v[k] & 0xFF0000u) ? 4u : 0u) |
                         ((v[k] & 0xFF000000u) ? 8u : 0u)) << (4 * k);
            s_any[w] = bits;
        }
        __syncthreads();
    }
    // The draw's housekeeping (no separate init kernel; these tables are idle now): zero the group rows of every entry-sort
    // pass, reset the bin ranges.
    {
        const uint32_t t = blockIdx.x * BIN_THREADS + threadIdx.x, stride = gridDim.x * BIN_THREADS;
        for (uint32_t w = t; w < (uint32_t)RADIX_TOTAL_WORDS; w += stride) digit_total[w] = 0u;
        for (uint32_t w = t; w < tiles; w += stride) tile_ranges[w] = make_uint2(0xFFFFFFFFu, 0u);
        // the chunked composite's per-draw words: no deep bins (k_bin_emit names them), an empty partial pool
        if (t < GS_FLAG_LIST) deep_flags[t] = 0u;
        for (uint32_t w = t; w < blend_bins; w += stride) deep_flags[GS_FLAG_OF + w] = GS_DEEP_NONE;
    }
    // the grid is sized for the host's count; a list whose real length only exists on the device (frustum-culled sort)
    // is spread over the same grid, and k_bin_emit learns the batches per workgroup from block_sums[3*BIN_MAX_BLOCKS]
    const uint32_t R = R_dev ? min(*R_dev, R_host) : R_host;
    const BinChunk ch = bin_chunk(R);
    BIN_PROF(0, 1, wall_clock64());
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t batches = (R + BIN_THREADS - 1) / BIN_THREADS;
        block_sums[3 * BIN_MAX_BLOCKS] = (batches + gridDim.x - 1) / gridDim.x;      // = bin_chunk()'s `per`
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t pos_begin = ch.begin * BIN_THREADS, pos_end = min(ch.end * BIN_THREADS, R);
    const SliceCount sc = bin_count_slice<NARROW>(order, R, perm, prect, rects, cidx, crect, coff, list_shift, splat_count, block_any, coarse, s_any, s_w, pos_begin, pos_end);
    uint32_t t16 = sc.t16;
    const uint32_t sum = sc.entries, out = pos_begin + sc.splats;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t16 += __shfl_xor(t16, o, 64);
    if (lane == 0) s_w[wave] = t16;                        // the loop's trailing barrier makes s_w reusable
    __syncthreads();
    if (threadIdx.x == 0) {
        block_sums[ch.id] = sum;
        block_sums[BIN_MAX_BLOCKS + ch.id] = out - pos_begin;
        block_sums[2 * BIN_MAX_BLOCKS + ch.id] = (uint32_t)(s_w[0] + s_w[1] + s_w[2] + s_w[3]);
    }
    BIN_PROF(0, 2, wall_clock64());
    BIN_PROF(0, 3, (unsigned long long)sum);
}

// What a lane reads of one live unit (draw_plan.hpp: a batch of <= 256 compacted splats of a slice that holds at least one): its
// splat's rect, record slot and first entry slot.  The three loads of a workgroup's NEXT unit are issued before this unit is
// expanded: a unit is loads -> arithmetic -> stores, and a workgroup's units are all known once its prologue is done.
struct EmitLoad {
    bool live;                 // the lane holds a splat (false for every lane: no such unit, or the draw overflowed before its slice)
    uint2 rect;                // 16-px tiles
    uint32_t idx, off, base;   // record slot | first entry slot = base (the slice's) + off (in the slice), added when the unit is expanded
};
// live_unit_find (draw_plan.hpp) by a wave over the words in LDS, every lane with the same answer: lane i asks the first slice of
// block i (LIVE_BLOCK slices: 33, so that the 64 reads fall into different banks), a ballot names the block; 34 lanes then read the
// block's slices and the next block's first one, and a second ballot names the slice.  Two LDS round trips instead of eleven.
constexpr uint32_t LIVE_BLOCK = 33;
static_assert((uint32_t)BIN_MAX_BLOCKS <= 64u * LIVE_BLOCK, "one lane per block of slices");
__device__ __forceinline__ LiveUnit live_unit_find_wave(const uint32_t* s_live, uint32_t slices, uint32_t total, uint32_t l) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i1 = lane * LIVE_BLOCK;
    const bool p1 = i1 < slices && (s_live[min(i1, slices - 1u)] & GS_LIVE_FIRST_MASK) <= l;
    const uint32_t block = (uint32_t)__popcll(__ballot(p1)) - 1u;                      // (slice 0's first is 0 <= l)
    const uint32_t i2 = block * LIVE_BLOCK + lane;
    const bool mine = lane <= LIVE_BLOCK && i2 < slices;
    const uint32_t w2 = mine ? s_live[min(i2, slices - 1u)] : 0u;
    const bool p2 = mine && lane < LIVE_BLOCK && (w2 & GS_LIVE_FIRST_MASK) <= l;
    const uint32_t in_block = (uint32_t)__popcll(__ballot(p2)) - 1u;                   // (the block's first slice has first <= l)
    const uint32_t slice = block * LIVE_BLOCK + in_block;
    const uint32_t word = __shfl(w2, (int)in_block, 64), after = __shfl(w2, (int)in_block + 1, 64);
    return live_unit_of(slice, word, slice + 1u < slices ? (after & GS_LIVE_FIRST_MASK) : total, l);
}

__device__ __forceinline__ EmitLoad bin_emit_load(const uint32_t* __restrict__ cidx, const uint2* __restrict__ crect, const uint32_t* __restrict__ coff,
                                                  const uint32_t* s_live, const uint32_t* s_eoff, uint32_t slices, uint32_t total, uint32_t per,
                                                  uint32_t l, uint32_t limit) {
    EmitLoad ld;
    ld.live = false; ld.rect = make_uint2(0u, 0u); ld.idx = 0u; ld.off = 0u; ld.base = 0u;
    if (l >= total) return ld;
    const LiveUnit u = live_unit_find_wave(s_live, slices, total, l);
    const uint32_t boff = s_eoff[u.slice];
    if (boff >= limit || threadIdx.x >= u.count) return ld;
    const uint32_t src = (u.slice * per + u.batch) * BIN_THREADS + threadIdx.x;   // the slice's part of the compacted lists
    ld.live = true;
    ld.rect = crect[src];
    ld.idx = cidx[src];
    ld.off = coff[src];
    ld.base = boff;
    return ld;
}

// One unit -> (list bin, record slot) entries: a lane writes the first EMIT_OWN entries of its own splat walking the rect row-major,
// what is left of the few splats that cover more list bins is written by the whole wave.  Returns the lane's entry count.
constexpr uint32_t EMIT_OWN = 16;      // entries a lane writes for its own splat; longer runs are shared by the wave
template <class KeyT>
__device__ __forceinline__ uint32_t bin_emit_batch(const EmitLoad ld, uint32_t limit, uint32_t tiles_x, uint32_t row_begin,
                                                   uint32_t list_shift, KeyT* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    const uint32_t lane = threadIdx.x & 63u;
    auto put = [&](uint32_t e, uint32_t key, uint32_t idx) {
        if (e >= limit) return;                              // dropped by an overflowing draw (it is redone)
        keys_out[e] = (KeyT)key;
        vals_out[e] = idx;
    };
    const uint2 r = rect_to_bins(ld.rect, list_shift);               // the list bins the splat touches
    const uint32_t idx = ld.idx, e0 = ld.base + ld.off, n = ld.live ? rect_tiles(r) : 0u;
    const uint32_t x0 = r.x & 0xFFFFu, y0 = r.x >> 16, w = (r.y & 0xFFFFu) - x0 + 1u;
    for (uint32_t k = 0, xx = x0, yy = y0; k < min(n, EMIT_OWN); k++) {     // row-major walk of the rect, no k / w, k % w
        put(e0 + k, (yy - row_begin) * tiles_x + xx, idx);
        if (++xx == x0 + w) { xx = x0; yy++; }
    }
    // the few near splats that cover many lists: all 64 lanes write one splat's remaining entries together
    unsigned long long big = __ballot(n > EMIT_OWN);
    while (big) {
        const int sl = __builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t bn = __shfl(n, sl, 64), be0 = __shfl(e0, sl, 64), bidx = __shfl(idx, sl, 64);
        const uint32_t bx0 = __shfl(x0, sl, 64), by0 = __shfl(y0, sl, 64), bw = __shfl(w, sl, 64);
        const float inv_w = 1.0f / (float)bw;
        for (uint32_t k = EMIT_OWN + lane; k < bn; k += 64u) {
            uint32_t q = (uint32_t)((float)k * inv_w);               // k / bw: k < 2^24, so the estimate is off by <= 1
            int32_t rem = (int32_t)(k - q * bw);
            if (rem < 0) { q--; rem += (int32_t)bw; }
            else if (rem >= (int32_t)bw) { q++; rem -= (int32_t)bw; }
            put(be0 + k, (by0 + q - row_begin) * tiles_x + bx0 + (uint32_t)rem, bidx);
        }
    }
    return n;
}

// The previous draw's per-bin statistics describe ITS view.  When the camera has moved since, the host says how far the scene's centre
// of mass moved on screen, in bins (draw_plan.cpp, plan_schedule): the schedule reads the statistics of the bin a bin's content came FROM - a camera
// that turns about its own position shifts the whole picture, and with it the costly bins and the deep pass's members, by that much.
struct StatShift {
    int32_t sx, sy;            // this draw's bin (bx, by) shows what the previous draw's bin (bx - sx, by - sy) showed
    uint32_t bins_x;
};
// The blend's schedule and the deep pass's members, one workgroup of BIN_THREADS (see where it is called: k_bin_emit)
// (prev_blend_stats and blend_stats_w are the same buffer - the previous draw's statistics, read, then the members' zeroed: no
// __restrict__ on either)
__device__ __forceinline__ void blend_schedule_job(const uint2* prev_blend_stats, uint32_t blend_bins, uint32_t* __restrict__ blend_order,
                                                   uint32_t deep, uint32_t* __restrict__ deep_flags, uint32_t* blend_stats_w,
                                                   uint32_t deep_min, uint32_t deep_factor, volatile uint32_t* __restrict__ mirror, StatShift sh,
                                                   uint32_t* s_tmp2 /* 4 words of LDS for the block scans */) {
    __shared__ uint32_t s_cost[RADIX_BINS];
    // (the chunked composite's per-draw words - no deep bins yet, an empty partial pool - were reset by k_bin_count, a kernel boundary ago)
    // three sweeps over the statistics, 8 loads in flight per lane (registers for all 8192 / 256 values would set the
    // whole kernel's VGPR allocation and cost every emitting workgroup its occupancy)
    constexpr uint32_t SWEEP = 8;
    auto cost_of = [&](uint32_t i) -> uint32_t {
        if (sh.sx == 0 && sh.sy == 0) return prev_blend_stats[i].y;
        const uint32_t by = i / sh.bins_x, bx = i - by * sh.bins_x;
        const int32_t fx = (int32_t)bx - sh.sx, fy = (int32_t)by - sh.sy;
        const uint32_t from = (uint32_t)fy * sh.bins_x + (uint32_t)fx;
        return (fx >= 0 && fy >= 0 && (uint32_t)fx < sh.bins_x && from < blend_bins) ? prev_blend_stats[from].y : 0u;
    };
    auto sweep = [&](auto&& use) {
        for (uint32_t base = 0; base < blend_bins; base += SWEEP * BIN_THREADS) {
            uint32_t c[SWEEP];
#pragma unroll
            for (uint32_t k = 0; k < SWEEP; k++) {
                const uint32_t i = base + threadIdx.x + k * BIN_THREADS;
                c[k] = i < blend_bins ? cost_of(i) : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < SWEEP; k++) {
                const uint32_t i = base + threadIdx.x + k * BIN_THREADS;
                if (i < blend_bins) use(i, c[k]);
            }
        }
    };
    uint32_t sum = 0;
    sweep([&](uint32_t, uint32_t c) { sum += c; });
    uint32_t total_walked;
    (void)block_excl_scan_256(sum, s_tmp2, &total_walked);
    // 8-bit cost key scaled to the scene: the mean bin lands near 48 whatever the scene walks per bin
    uint32_t shift = 0;
    while (((total_walked / blend_bins) >> shift) > 48u) shift++;
    s_cost[threadIdx.x] = 0u;
    __syncthreads();
    sweep([&](uint32_t, uint32_t c) { atomicAdd(&s_cost[255u - min(c >> shift, 255u)], 1u); });
    __syncthreads();
    const uint32_t cnt_d = s_cost[threadIdx.x];
    const uint32_t start = block_excl_scan_256(cnt_d, s_tmp2, nullptr);
    s_cost[threadIdx.x] = start;
    __syncthreads();
    sweep([&](uint32_t i, uint32_t c) { blend_order[atomicAdd(&s_cost[255u - min(c >> shift, 255u)], 1u)] = i; });
    // The deep pass (tile_blend.hip): among the GS_DEEP_MAX_BINS costliest bins (the head of the order just written), the ones
    // whose previous draw walked >= deep_min (splat, quadrant) pairs are composited by one wave per (quadrant, chunk) + a fold
    // instead of by one workgroup - same pixels either way, so this is scheduling only.  Their count goes to the host (the NEXT
    // draw launches the deep pass when it is non-zero); they are only named when THIS draw runs the pass.  Their statistics
    // are then summed atomically by many waves: zeroed here.
    // (a bin qualifies when it walked >= deep_min pairs AND >= deep_factor x the mean bin: the pass costs three launches, and
    // only a tail that is long against the body of the frame pays for them - C3T's costliest bins are 3 x its mean and gain
    // nothing, C3S's are 18 x; .y = half quadrants evaluated = 2 per pair, total_walked is their sum)
    // Once the pass runs, more bins in it cost next to nothing, and every bin left behind is a workgroup that walks alone at the
    // end of the launch: membership starts at 3/4 of the mean (and never below deep_min).
    const uint32_t mean_halves = total_walked / max(blend_bins, 1u);
    const uint32_t deep_trigger = max(2u * deep_min, deep_factor * mean_halves), deep_thr = max(2u * deep_min, mean_halves - mean_halves / 4u);
    __shared__ uint32_t s_trigger;
    if (threadIdx.x == 0) s_trigger = 0u;
    __shared__ uint32_t s_deep_n, s_deep_cost;
    if (threadIdx.x == 0) { s_deep_n = 0u; s_deep_cost = 0u; }
    __threadfence_block();
    __syncthreads();                                   // blend_order complete (and visible to this workgroup)
    // Two phases: every member is decided before any statistics are zeroed.  blend_stats_w IS prev_blend_stats, and with a
    // StatShift a bin's cost is read from ANOTHER bin (a neighbour, which may be a member): zeroing in the same loop made later
    // readers - other threads, and this thread's second head position - see 0 and drop bins from the pass.
    constexpr uint32_t HEAD_PER_T = (GS_DEEP_MAX_BINS + BIN_THREADS - 1u) / BIN_THREADS;
    uint32_t member[HEAD_PER_T];
#pragma unroll
    for (uint32_t q = 0; q < HEAD_PER_T; q++) {
        const uint32_t p = threadIdx.x + q * BIN_THREADS;
        member[q] = GS_DEEP_NONE;
        if (p >= min(blend_bins, GS_DEEP_MAX_BINS)) continue;
        const uint32_t i = __hip_atomic_load(&blend_order[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t cost = i < blend_bins ? cost_of(i) : 0u;
        if (cost >= deep_trigger) s_trigger = 1u;
        if (cost >= deep_thr) {
            const uint32_t k = atomicAdd(&s_deep_n, 1u);
            atomicAdd(&s_deep_cost, cost >> 4);            // (the members' share of the frame's walk: sixteenths, < 2^32 for any frame)
            if (deep) {
                deep_flags[GS_FLAG_LIST + k] = i;
                deep_flags[GS_FLAG_OF + i] = k;
                member[q] = i;
            }
        }
    }
    __syncthreads();                                   // every cost_of() of the head has been read
#pragma unroll
    for (uint32_t q = 0; q < HEAD_PER_T; q++) {
        const uint32_t i = member[q];
        if (i != GS_DEEP_NONE) { blend_stats_w[2u * i] = 0u; blend_stats_w[2u * i + 1u] = 0u; blend_stats_w[2u * blend_bins + i] = 0u; }
    }
    if (threadIdx.x == 0) {
        // (a draw whose tail no longer reaches the trigger still runs the pass it was launched with - on the bins of the
        // membership rule - and tells the next one to stop)
        deep_flags[GS_FLAG_CAND] = s_trigger ? s_deep_n : 0u;
        if (deep) deep_flags[GS_FLAG_COUNT] = s_deep_n;
        if (mirror) {
            mirror[GS_MIRROR_DEEP_CANDIDATES] = s_trigger ? s_deep_n : 0u;
            // ... and what share of the previous draw's walk those bins were, in 1 / 1024: how many of the blend's workgroups the pass
            // should get (tile_blend.hip, gs_launch_blend)
            mirror[GS_MIRROR_DEEP_SHARE] = (uint32_t)(((unsigned long long)s_deep_cost << 14) / (unsigned long long)max(total_walked, 1u));
        }
    }
}

// k_bin_emit: splat-centric expansion of the compacted list into (list bin, record slot) pairs.
// Work unit = one batch of 256 compacted splats of one binning workgroup's slice that holds at least one splat (a live unit,
// draw_plan.hpp); the units are dealt round-robin to the workgroups.  (Dealing every (slice, batch) pair, empty or not, gave the
// workgroups of one residue class most of the live ones: C3 has 12 batches per slice of which the first three or four are live, and
// 2048 workgroups step through the pairs by 2048 mod 12 = 8, so a workgroup only ever met the batch indices {r, r + 4, r + 8} - a
// quarter of the grid expanded 4.7 live batches each, the rest 2 to 3.3, and the kernel lasted as long as the former:
// profiles/r13_emit_timeline_before.txt.)  (One workgroup per binning workgroup, the r01 shape, lasted as long as its heaviest slice: the slices that hold
// the nearest splats carry 30x the mean entry count - r02n timeline: mean workgroup 8 us, last one 27 us, and the same 27 us
// for a strip-sharded rank that emits an eighth of the entries.)  A lane writes the first OWN entries of its splat itself,
// walking the rect row-major; what is left of the few splats that cover more list bins is written by the whole wave.
// block_sums: [0,BIN_MAX_BLOCKS) entries of every binning workgroup | [BIN_MAX_BLOCKS,..) its compacted splat count |
// [2*BIN_MAX_BLOCKS,..) its 16-px tiles | [3*BIN_MAX_BLOCKS] batches per binning workgroup.
// Every workgroup scans the binning workgroups' sums itself (8 KB of hot L2 lines: cheaper than a one-workgroup scan kernel
// and its two kernel boundaries); workgroup 0 publishes the RenderFrame scalars that the following kernels read.
template <class KeyT>
__global__ __launch_bounds__(BIN_THREADS) void k_bin_emit(RenderFrame* __restrict__ frame, uint32_t capacity,
                                                          const uint32_t* __restrict__ cidx,
                                                          const uint2* __restrict__ crect, const uint32_t* __restrict__ coff,
                                                          const uint32_t* __restrict__ block_sums, uint32_t bin_grid,
                                                          uint32_t tiles_x /* list bins per row */,
                                                          uint32_t row_begin /* first list-bin row */, KeyT* __restrict__ keys_out,
                                                          uint32_t* __restrict__ vals_out, uint32_t list_shift,
                                                          volatile uint32_t* __restrict__ mirror, uint32_t serial,
                                                          const uint2* prev_blend_stats, uint32_t blend_bins,
                                                          uint32_t* __restrict__ blend_order, uint32_t deep,
                                                          uint32_t* __restrict__ deep_flags, uint32_t* blend_stats_w,
                                                          uint32_t deep_min, uint32_t deep_factor, StatShift sh) {
    __shared__ __attribute__((aligned(16))) uint32_t s_eoff[BIN_MAX_BLOCKS];   // entries of the binning workgroups before b (saturating)
    __shared__ __attribute__((aligned(16))) uint32_t s_live[BIN_MAX_BLOCKS];   // live batches before b | its last batch's splats (draw_plan.hpp, live_unit_word)
    __shared__ unsigned long long s_wsum[4], s_t16[4];
    __shared__ uint32_t s_vis[4], s_lsum[4];                                   // (s_lsum: the schedule job's scan scratch as well)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    BIN_PROF(1, 0, wall_clock64());
    BIN_PROF(1, 2, 0ull);
    // Blend schedule of THIS draw, by one extra workgroup (the first to be dispatched): the 32-px bins in descending order of
    // what they cost in the PREVIOUS draw ((splat, tile) pairs walked, k_tile_blend's per-bin statistics).  Every bin of a 1080p
    // frame is resident at once and a SIMD's time is the sum of its waves' walks, so the kernel used to last ~2x its mean bin
    // (r02g counters: VALU busy 39 % of the launch, ~all of the time while 8 waves are resident); heavy bins first + fewer
    // resident workgroups lets the cheap ones backfill.  A counting sort of <= 8 k keys held in registers; the order of equal
    // keys is irrelevant (pixels do not depend on which workgroup draws a bin).
    const uint32_t first_wg = blend_order ? 1u : 0u;
    if (blend_order && blockIdx.x == 0) {
        blend_schedule_job(prev_blend_stats, blend_bins, blend_order, deep, deep_flags, blend_stats_w, deep_min, deep_factor, mirror, sh, s_lsum);
        BIN_PROF(1, 1, wall_clock64());
        BIN_PROF(1, 2, wall_clock64());
        return;
    }
    const uint32_t wg = blockIdx.x - first_wg, wgs = gridDim.x - first_wg;
    // exclusive scan of the binning workgroups' entry sums: thread t owns the PER_T consecutive sums [t * PER_T, ..), read
    // with 16-byte loads (block_sums rows are 16-byte aligned)
    constexpr uint32_t PER_T = BIN_MAX_BLOCKS / BIN_THREADS;
    static_assert(PER_T % 4 == 0, "16-byte loads of the workgroup sums");
    uint32_t mine[PER_T], cnt[PER_T];
    unsigned long long own = 0;
    uint32_t own_live = 0;
#pragma unroll
    for (uint32_t q = 0; q < PER_T / 4; q++) {
        const uint32_t i0 = threadIdx.x * PER_T + 4 * q;
        const uint4 e = reinterpret_cast<const uint4*>(block_sums)[i0 / 4];
        uint4 c = reinterpret_cast<const uint4*>(block_sums + BIN_MAX_BLOCKS)[i0 / 4];
        mine[4 * q + 0] = i0 + 0 < bin_grid ? e.x : 0u;
        mine[4 * q + 1] = i0 + 1 < bin_grid ? e.y : 0u;
        mine[4 * q + 2] = i0 + 2 < bin_grid ? e.z : 0u;
        mine[4 * q + 3] = i0 + 3 < bin_grid ? e.w : 0u;
        c.x = i0 + 0 < bin_grid ? c.x : 0u;
        c.y = i0 + 1 < bin_grid ? c.y : 0u;
        c.z = i0 + 2 < bin_grid ? c.z : 0u;
        c.w = i0 + 3 < bin_grid ? c.w : 0u;
        cnt[4 * q + 0] = c.x; cnt[4 * q + 1] = c.y; cnt[4 * q + 2] = c.z; cnt[4 * q + 3] = c.w;
    }
#pragma unroll
    for (uint32_t k = 0; k < PER_T; k++) { own += mine[k]; own_live += live_batches(cnt[k]); }
    const unsigned long long incl = wave_incl_scan(own, lane);
    const uint32_t incl_live = wave_incl_scan(own_live, lane);
    if (lane == 63u) { s_wsum[wave] = incl; s_lsum[wave] = incl_live; }
    __syncthreads();
    unsigned long long run = incl - own, D64 = 0;
    uint32_t run_live = incl_live - own_live, L = 0;         // live batches before this thread's slices | of the draw
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const unsigned long long c = s_wsum[w];
        run += w < wave ? c : 0ull;
        D64 += c;
        const uint32_t cl = s_lsum[w];
        run_live += w < wave ? cl : 0u;
        L += cl;
    }
#pragma unroll
    for (uint32_t q = 0; q < PER_T / 4; q++) {
        uint32_t v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            v[k] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
            run += mine[4 * q + k];
        }
        reinterpret_cast<uint4*>(s_eoff)[(threadIdx.x * PER_T + 4 * q) / 4] = make_uint4(v[0], v[1], v[2], v[3]);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            v[k] = live_unit_word(run_live, cnt[4 * q + k]);
            run_live += live_batches(cnt[4 * q + k]);
        }
        reinterpret_cast<uint4*>(s_live)[(threadIdx.x * PER_T + 4 * q) / 4] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    const uint32_t D = D64 > capacity ? capacity : (uint32_t)D64;
    if (wg == 0) {                                           // the frame's scalars (read by the sort passes and the host)
        unsigned long long t16 = 0;
        uint32_t vis = 0;
        for (uint32_t i = threadIdx.x; i < bin_grid; i += BIN_THREADS) {
            vis += block_sums[BIN_MAX_BLOCKS + i];
            t16 += block_sums[2 * BIN_MAX_BLOCKS + i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            vis += __shfl_xor(vis, o, 64);
            t16 += __shfl_xor(t16, o, 64);
        }
        if (lane == 0u) { s_t16[wave] = t16; s_vis[wave] = vis; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long tsum = s_t16[0] + s_t16[1] + s_t16[2] + s_t16[3];
            frame->tiles16_lo = (uint32_t)tsum;
            frame->tiles16_hi = (uint32_t)(tsum >> 32);
            frame->visible = s_vis[0] + s_vis[1] + s_vis[2] + s_vis[3];
            frame->entries_lo = (uint32_t)D64;
            frame->entries_hi = (uint32_t)(D64 >> 32);
            frame->overflow = D64 > capacity ? 1u : 0u;
            frame->entry_count = D;
            frame->pad = 0;
            // host-visible copy of the overflow verdict (mapped pinned memory): an asynchronous draw that ran out of entry
            // slots is noticed by the NEXT gs_mesh_render without a synchronisation (mesh.hip, mesh_heal_overflow).
            // One 16-byte store = one PCIe write: the four words land together, no system-scope fence between them
            if (mirror) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 v = {serial, D64 > capacity ? 1u : 0u, (uint32_t)D64, (uint32_t)(D64 >> 32)};
                *reinterpret_cast<volatile u32x4*>(mirror + GS_MIRROR_SERIAL) = v;
                // ... and, as a second 16-byte store, {serial, visible splats, 16-px tiles they touch}: what tells the following draws how
                // much of the scene is in view (project.hip: where the block test runs) and how large its splats are on screen (the size
                // of the list bins, draw_plan.cpp: adapt_list_shift) without anybody asking for statistics
                const u32x4 sv = {serial, s_vis[0] + s_vis[1] + s_vis[2] + s_vis[3], (uint32_t)tsum, (uint32_t)(tsum >> 32)};
                *reinterpret_cast<volatile u32x4*>(mirror + GS_MIRROR_VIEW_SERIAL) = sv;
            }
        }
    }
    __syncthreads();                                         // s_eoff and s_live complete
    BIN_PROF(1, 1, wall_clock64());
    const uint32_t per = block_sums[3 * BIN_MAX_BLOCKS];     // batches per binning workgroup (k_bin_count)
    // the draw's L live units, round-robin (draw_plan.hpp); the next unit's loads fly while this one is expanded
    uint32_t emitted = 0, walked = 0;
    EmitLoad cur = bin_emit_load(cidx, crect, coff, s_live, s_eoff, bin_grid, L, per, wg, D);
    // (the first unit's loads are awaited HERE: left to the compiler, their wait lands in the loop, behind the next unit's loads -
    // the counter is in order - and every iteration waits for the loads it has just issued.  vmcnt(0), the other counters untouched)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (uint32_t l = wg; l < L; l += wgs) {
        const EmitLoad next = bin_emit_load(cidx, crect, coff, s_live, s_eoff, bin_grid, L, per, l + wgs, D);
        emitted += bin_emit_batch<KeyT>(cur, D, tiles_x, row_begin, list_shift, keys_out, vals_out);
        cur = next;
        walked++;
    }
    BIN_PROF(1, 2, wall_clock64());
    BIN_PROF(1, 3, (unsigned long long)emitted | ((unsigned long long)walked << 32));
    (void)emitted; (void)walked;
}

// what plan_schedule (draw_plan.hpp) is told about this draw, the mesh and the draw before
static ScheduleInputs schedule_inputs(const gs_mesh* m, const DrawSwitches& sw, const DrawFeedback& fb, const ProjectParams& pp) {
    ScheduleInputs in;
    in.stats = m->stats_of;
    in.now = plan_view(pp);
    in.bins_x = pp.bins_x; in.bin_row_begin = pp.bin_row_begin; in.bin_row_end = pp.bin_row_end;
    in.block_cull = pp.block_cull;
    in.draw_mode = m->draw_mode;
    in.draw_serial = m->draw_serial;
    in.no_deep = m->no_deep;
    memcpy(in.centre_sum, m->centre_sum, sizeof(in.centre_sum));
    in.centre_n = m->centre_n;
    in.feedback = fb;
    in.sw = sw;
    return in;
}

template <class KeyT>
static int binning_typed(gs_mesh* m, const DrawSwitches& sw, const DrawFeedback& fb, const ProjectParams& pp, const uint32_t* order_dev, gs_sorter* sorter, uint32_t R, uint32_t tiles /* sort keys */) {
    gs_context* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const ProjSet& ps = m->set();                           // the set this draw's vertex stage wrote
    const RadixExec ex = {st, &m->radix, ctx->lds_atomic_lane_order};
    RenderFrame* frame = m->frame.as<RenderFrame>();
    uint32_t grid = (R + BIN_THREADS - 1) / BIN_THREADS;
    if (grid < 1) grid = 1;
    if (grid > (uint32_t)BIN_MAX_BLOCKS) grid = BIN_MAX_BLOCKS;
    const uint32_t cap = m->entry_capacity;
    const uint32_t* R_dev = (sorter && sorter->last_plan.count_on_device) ? &sorter->result_frame->kept : nullptr;
    const uint32_t blend_bins = pp.bins_x * (pp.bin_row_end - pp.bin_row_begin);
    // the chunked composite's per-draw words and the pool the per-bin kernel closes chunks into (reset by k_bin_count)
    GS_TRY(m->deep_flags.ensure(((size_t)GS_FLAG_OF + blend_bins) * 4 + 64));
    GS_TRY(m->chunk_pool.ensure((size_t)GS_POOL_SLOTS * 256 * sizeof(float4)));
    GS_TRY(m->blend_stats.ensure((size_t)blend_bins * 12));
    if (sorter && sorter->stream != st) {      // the sorter's private stream may overwrite `sorted` from here on
        GS_HIP(hipEventRecord(sorter->ev_consumed, st));
        sorter->consumer_pending = true;
    }
    // whether the previous draw's statistics order this draw's bins (read shifted by how many bins), and whether the deep pass
    // runs: draw_plan.cpp (the result is kept for gs_launch_blend and gs_mesh_debug_read(what = 7))
    m->plan = plan_schedule(schedule_inputs(m, sw, fb, pp));
    const SchedulePlan& plan = m->plan;
    if (plan.order_ok) GS_TRY(m->blend_order.ensure((size_t)blend_bins * 4));
    if (plan.deep_pass) {
        GS_TRY(m->deep_ent.ensure((size_t)GS_DEEP_MAX_BINS * GS_DEEP_LIST_CAP * 4));
        GS_TRY(m->deep_cnt.ensure((size_t)GS_DEEP_MAX_BINS * GS_DEEP_RANGES * 4 * 4));
        GS_TRY(m->deep_partial.ensure((size_t)GS_DEEP_UNITS * 256 * sizeof(float4)));
        GS_TRY(m->deep_work.ensure((size_t)GS_DEEP_UNITS * 4));
    }
    const bool order_wg = plan.order_wg;
    const StatShift stat_shift = {plan.sx, plan.sy, pp.bins_x};
    ++m->draw_serial;
    if (m->draw_serial == 0u) m->draw_serial = 1u;       // (the mapped words carry the serial: 0 is "no draw yet", mesh_read_view_share)
    // (the word the vertex stage wrote into this set: mesh.hip, mesh_project)
    auto count_pass = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(BIN_THREADS), 0, st, order_dev, R, R_dev,
                           m->translate ? m->perm.as<uint32_t>() : nullptr, ps.prect.p, ps.rects.as<uint2>(), m->cidx.as<uint32_t>(), m->rect_q.as<uint2>(), m->coff.as<uint32_t>(),
                           m->bin_sums.as<uint32_t>(), m->radix.digit_total.as<uint32_t>(),
                           m->tile_ranges.as<uint2>(), tiles, pp.list_shift, pp.count,
                           ps.block_any.as<uint8_t>(), m->deep_flags.as<uint32_t>(), blend_bins, m->no_coarse_vis ? 0u : 1u);
    };
    if (ps.narrow_word) count_pass(k_bin_count<true>);
    else count_pass(k_bin_count<false>);
    hipLaunchKernelGGL((k_bin_emit<KeyT>), dim3(grid + (order_wg ? 1u : 0u)), dim3(BIN_THREADS), 0, st, frame, cap, m->cidx.as<uint32_t>(),
                       m->rect_q.as<uint2>(), m->coff.as<uint32_t>(), m->bin_sums.as<uint32_t>(), grid, pp.lists_x, pp.list_row_begin,
                       m->ekeyA.as<KeyT>(), m->evalA.as<uint32_t>(), pp.list_shift, m->mirror_dev, m->draw_serial,
                       order_wg ? m->blend_stats.as<uint2>() : nullptr, blend_bins, order_wg ? m->blend_order.as<uint32_t>() : nullptr,
                       plan.deep_pass ? 1u : 0u, m->deep_flags.as<uint32_t>(), m->blend_stats.as<uint32_t>(), plan.deep_min, plan.deep_factor, stat_shift);
    GS_HIP(hipGetLastError());
    if (pp.row_begin == 0u && pp.row_end >= pp.tiles_y) {     // (a strip's visible count says nothing about the scene: mesh_heal_overflow)
        m->full_serial[m->draw_serial & 7u] = m->draw_serial;
        m->full_count[m->draw_serial & 7u] = pp.count;
    }
    if (m->timed_draw) GS_HIP(hipEventRecord(m->ev[2], st));

    uint32_t bits = 1;
    while ((1ull << bits) < tiles) bits++;
    const uint32_t passes = (bits + 7) / 8;
    KeyT* kbuf[2] = {m->ekeyA.as<KeyT>(), m->ekeyB.as<KeyT>()};
    uint32_t* vbuf[2] = {m->evalA.as<uint32_t>(), m->evalB.as<uint32_t>()};
    for (uint32_t p = 0; p < passes; p++) {
        ArrayLoader<KeyT> al = {kbuf[p & 1], vbuf[p & 1], &frame->entry_count, 0u};
        if (passes == 1)                           // <= 256 lists: the digit is the key, ranges come from the digit totals
            GS_TRY((radix_pass<ArrayLoader<KeyT>, KeyT, false, false>(ex, al, al, cap, 0, 0, (KeyT*)nullptr, vbuf[1],
                                                                      m->tile_ranges.as<uint2>(), tiles)));
        else if (p + 1 == passes)
            GS_TRY((radix_pass<ArrayLoader<KeyT>, KeyT, false, true>(ex, al, al, cap, 8 * (int)p, (int)p, (KeyT*)nullptr,
                                                                     vbuf[(p + 1) & 1], m->tile_ranges.as<uint2>())));
        else
            GS_TRY((radix_pass<ArrayLoader<KeyT>, KeyT, true, false>(ex, al, al, cap, 8 * (int)p, (int)p, kbuf[(p + 1) & 1],
                                                                     vbuf[(p + 1) & 1])));
    }
    m->sorted_buf = (passes & 1);            // which ping-pong buffer holds the tile-sorted entries
    return GS_OK;
}

int gs_launch_binning(gs_mesh* m, const DrawSwitches& sw, const DrawFeedback& fb, const ProjectParams& pp, const uint32_t* order_dev, gs_sorter* sorter, uint32_t render_count) {
    const uint32_t tiles = pp.lists_x * (pp.list_row_end - pp.list_row_begin);   // one list per sort key
    if (tiles <= 65536u && !m->ctx->wide_entry_keys) return binning_typed<uint16_t>(m, sw, fb, pp, order_dev, sorter, render_count, tiles);
    return binning_typed<uint32_t>(m, sw, fb, pp, order_dev, sorter, render_count, tiles);
}
