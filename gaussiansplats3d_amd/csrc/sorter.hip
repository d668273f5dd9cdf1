// sorter.hip — the SORT SEAM on gfx950: replaces the reference's Web-Worker + WASM counting sort
// (/root/reference/src/worker/SortWorker.js:31-81 -> sorter.cpp:17-168) with
//   k_depth_key      phase A  per-splat int32 view-depth key + device-wide min/max   (sorter.cpp:29-140)
//   radix passes     phase B-D bucket mapping fused into pass 0 of a stable LSD radix sort over
//                    key' = range-1-bucket of the REVERSED list, which reproduces the reference's output
//                    order exactly: buckets far->near, equal buckets in reverse input order
//                    (sorter.cpp:142-167).
// What one sort launches - which front end, on which grids, what every radix pass reads and writes - is decided before anything is
// enqueued, by plan_sort (sort_plan.cpp: host only, held to a host model by tests/test_sort_plan.py); the host code at the end of
// this file gathers the plan's inputs, runs the refusals and acts on the plan.
// Arithmetic that decides the order is spelled with non-contracting intrinsics (__fmul_rn ...) so hipcc's
// default fp-contract=fast cannot fuse it; this file is also built with -ffp-contract=off.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "extreme_set.hpp"
#include "radix.hpp"

// WASM (emscripten) float->int: NaN / out of range -> INT32_MIN (same rule as oracle/sort_oracle.c)
__host__ __device__ static inline int32_t trunc_f64_i32(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return INT32_MIN;
    return (int32_t)v;
}

constexpr uint32_t MODE_INT = 1, MODE_DYNAMIC = 2, MODE_PRECOMPUTED = 4;

struct SceneRows {                 // per-scene clip-z row (mvp * transform)[2], as int x1000 and as float
    int32_t im[GS_MAX_SCENES][4];
    float fm[GS_MAX_SCENES][4];
};

struct KeyParams {
    const uint32_t *cx, *cy, *cz, *cw;       // SoA planes (int32 or float bit patterns): streaming (identity list) path
    const uint4* aos;                        // the same centres as uploaded (x,y,z,w): ONE 16-byte gather per index
    const uint32_t* scene_idx;
    const uint32_t* idx_in;                  // nullable: identity
    const uint32_t* precomputed;             // int32 or float bit patterns
    const SceneRows* rows;
    int32_t* keys_out;
    SortFrame* frame;                        // min / max / clamp counter of THIS sort (pre-initialised, see below)
    SortFrame* next_frame;                   // the other buffer: reset here for the next sort (no separate init kernel)
    uint32_t* digit_total;                   // radix digit totals of this sort's passes: zeroed here, before any histogram
    uint32_t sort_start, render_count, mode;
    uint32_t last_splat;                     // uploaded - 1: list entries are clamped to it (the reference reads whatever
                                             // WASM memory a stale index points at; here that would be a GPU page fault)
    int32_t im0, im1, im2;                   // static path: (int)(mvp[k]*1000.0), k = 2,6,10
    float fm0, fm1, fm2;                     // static float path: mvp[2], mvp[6], mvp[10]
    float mvp[16];                           // frustum-cull variant only: the whole modelViewProj, fp32 column-major
    unsigned long long* keep;                // cull variants only: 1 bit per list position
    const uint32_t* count_dev;               // visibility-cull variant: the list length lives on the device (SortFrame::kept)
    uint32_t ext_minmax;                     // ... and min / max (over EVERY splat) were taken by k_minmax_count: leave them alone
};

// The per-scene rows of a dynamic sort travel as a kernel ARGUMENT (1 KB of kernarg, captured when the launch is enqueued),
// so the host copy may die with the caller's stack frame and the sort stays asynchronous.
__global__ __launch_bounds__(256) void k_store_scene_rows(SceneRows rows, SceneRows* __restrict__ dst) {
    const uint32_t t = threadIdx.x;
    if (t < GS_MAX_SCENES * 4) {
        dst->im[t >> 2][t & 3] = rows.im[t >> 2][t & 3];
        dst->fm[t >> 2][t & 3] = rows.fm[t >> 2][t & 3];
    }
}

__global__ __launch_bounds__(256) void k_aos4_to_soa(const uint4* __restrict__ aos, uint32_t count, uint32_t from,
                                                     uint32_t* __restrict__ x, uint32_t* __restrict__ y,
                                                     uint32_t* __restrict__ z, uint32_t* __restrict__ w) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const uint4 v = aos[i];
        x[from + i] = v.x;
        y[from + i] = v.y;
        z[from + i] = v.z;
        if (w) w[from + i] = v.w;
    }
}

// The 16-bit offset planes of positions [from, end) from the int32 planes: d = c - o per axis (int64: centres sit anywhere in int32).
// Every d must lie in [0, 65535]; the ones that do not are counted into *bad (and stored truncated - the host refuses the planes
// when the count is not 0, so nothing ever reads them).
__global__ __launch_bounds__(256) void k_compact_centres(const int32_t* __restrict__ x, const int32_t* __restrict__ y,
                                                         const int32_t* __restrict__ z, uint32_t from, uint32_t end, int32_t ox, int32_t oy,
                                                         int32_t oz, uint16_t* __restrict__ x16, uint16_t* __restrict__ y16,
                                                         uint16_t* __restrict__ z16, uint32_t* __restrict__ bad) {
    uint32_t nbad = 0;
    for (uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) {
        const int64_t dx = (int64_t)x[i] - ox, dy = (int64_t)y[i] - oy, dz = (int64_t)z[i] - oz;
        nbad += (dx < 0 || dx > 65535 || dy < 0 || dy > 65535 || dz < 0 || dz > 65535) ? 1u : 0u;
        x16[i] = (uint16_t)dx;
        y16[i] = (uint16_t)dy;
        z16[i] = (uint16_t)dz;
    }
    if (nbad) atomicAdd(bad, nbad);
}

// ---------------------------------------------------------------------------------------------------
// The rules every front-end kernel shares, each said once: the static key, the centre as the frustum test sees it, the
// housekeeping of a sort's first kernel, the min / max accumulator.
// ---------------------------------------------------------------------------------------------------
// The static key of one centre (three words of its plane / AoS entry), integer mode: int32 wrap-around.  sorter.cpp:63-75
__device__ __forceinline__ int32_t static_key_int(const KeyParams& p, uint32_t x, uint32_t y, uint32_t z) {
    return (int32_t)(x * (uint32_t)p.im0 + y * (uint32_t)p.im1 + z * (uint32_t)p.im2);
}
// ... float mode: fp32 left to right, no contraction, then x4096 in double and WASM's truncation.  sorter.cpp:128-138
__device__ __forceinline__ int32_t static_key_float(const KeyParams& p, uint32_t xb, uint32_t yb, uint32_t zb) {
    float s = __fmul_rn(p.fm0, __uint_as_float(xb));
    s = __fadd_rn(s, __fmul_rn(p.fm1, __uint_as_float(yb)));
    s = __fadd_rn(s, __fmul_rn(p.fm2, __uint_as_float(zb)));
    return trunc_f64_i32((double)s * 4096.0);
}
__device__ __forceinline__ int32_t static_key(const KeyParams& p, uint32_t x, uint32_t y, uint32_t z) {
    return (p.mode & MODE_INT) ? static_key_int(p, x, y, z) : static_key_float(p, x, y, z);
}
// ... of position i of the SoA planes (the loads inside the mode branch)
__device__ __forceinline__ int32_t static_key_planes(const KeyParams& p, uint32_t i) {
    if (p.mode & MODE_INT) return static_key_int(p, p.cx[i], p.cy[i], p.cz[i]);
    return static_key_float(p, p.cx[i], p.cy[i], p.cz[i]);
}
// four consecutive splats, one 16-byte vector per plane (integer mode)
__device__ __forceinline__ int4 static_key_int4(const KeyParams& p, const uint4& x, const uint4& y, const uint4& z) {
    return make_int4(static_key_int(p, x.x, y.x, z.x), static_key_int(p, x.y, y.y, z.y), static_key_int(p, x.z, y.z, z.z),
                     static_key_int(p, x.w, y.w, z.w));
}

// The centre as the frustum test (frustum_keep_one) sees it: the sorter's own centre words as floats.
__device__ __forceinline__ float3 centre_int_as_float(uint32_t x, uint32_t y, uint32_t z) {
    return make_float3(__fmul_rn((float)(int32_t)x, 0.001f), __fmul_rn((float)(int32_t)y, 0.001f), __fmul_rn((float)(int32_t)z, 0.001f));
}
// ... and the static key with it, in ONE mode branch (c: a gathered centre)
__device__ __forceinline__ int32_t static_key_centre(const KeyParams& p, const uint4& c, float3& centre) {
    if (p.mode & MODE_INT) {
        centre = centre_int_as_float(c.x, c.y, c.z);
        return static_key_int(p, c.x, c.y, c.z);
    }
    centre = make_float3(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z));
    return static_key_float(p, c.x, c.y, c.z);
}

// The dynamic key of one centre (x, y, z, w: its four words as uploaded - w is whatever the caller sent, not a constant) and the
// row of its scene (four words of SceneRows::im or ::fm, the mode's).  Integer mode: uint32 wrap-around (sorter.cpp:41-62);
// float mode: fp32 left to right, no contraction, then x4096 in double and WASM's truncation (:110-126).
__device__ __forceinline__ int32_t dynamic_key(uint32_t mode, const uint4& r, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    if (mode & MODE_INT) return (int32_t)(x * r.x + y * r.y + z * r.z + w * r.w);
    float s = __fmul_rn(__uint_as_float(r.x), __uint_as_float(x));
    s = __fadd_rn(s, __fmul_rn(__uint_as_float(r.y), __uint_as_float(y)));
    s = __fadd_rn(s, __fmul_rn(__uint_as_float(r.z), __uint_as_float(z)));
    s = __fadd_rn(s, __fmul_rn(__uint_as_float(r.w), __uint_as_float(w)));
    return trunc_f64_i32((double)s * 4096.0);
}
// The row of scene `si` in the mode in use, as four words.  An index beyond the table is masked into it: the key of such a splat
// is unspecified, the read is not.
static_assert((GS_MAX_SCENES & (GS_MAX_SCENES - 1)) == 0, "scene indexes are masked into the table");
__device__ __forceinline__ uint4 scene_row(const SceneRows* rows, uint32_t mode, uint32_t si) {
    si &= GS_MAX_SCENES - 1u;
    if (mode & MODE_INT) {
        const int32_t* r = rows->im[si];
        return make_uint4((uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[2], (uint32_t)r[3]);
    }
    const float* r = rows->fm[si];
    return make_uint4(__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3]));
}
// ... for the streaming kernels of a dynamic sort: the 32 rows of the mode in use, staged in LDS once per workgroup (512 bytes;
// the caller's next barrier publishes them)
__device__ __forceinline__ void stage_scene_rows(const KeyParams& p, uint4* s_rows) {
    if (threadIdx.x < GS_MAX_SCENES) s_rows[threadIdx.x] = scene_row(p.rows, p.mode, threadIdx.x);
}
// four consecutive splats of the planes (x, y, z, w, scene index: one 16-byte vector each), rows from LDS
__device__ __forceinline__ int4 dynamic_key4(uint32_t mode, const uint4* s_rows, const uint4& x, const uint4& y, const uint4& z,
                                             const uint4& w, const uint4& si) {
    constexpr uint32_t M = GS_MAX_SCENES - 1u;
    return make_int4(dynamic_key(mode, s_rows[si.x & M], x.x, y.x, z.x, w.x), dynamic_key(mode, s_rows[si.y & M], x.y, y.y, z.y, w.y),
                     dynamic_key(mode, s_rows[si.z & M], x.z, y.z, z.z, w.z), dynamic_key(mode, s_rows[si.w & M], x.w, y.w, z.w, w.w));
}

// Every mode, for the splat a list entry names: precomputed and dynamic keys, else the static key of its gathered centre.
__device__ __forceinline__ int32_t depth_key_one(const KeyParams& p, uint32_t g) {
    if (p.mode & MODE_PRECOMPUTED) {
        const uint32_t raw = p.precomputed[g];
        if (p.mode & MODE_INT) return (int32_t)raw;                                        // sorter.cpp:31-38
        return trunc_f64_i32((double)__uint_as_float(raw) * 4096.0);                       // :79-86
    }
    const uint4 c = p.aos[g];                                                              // gathered by list index
    if (!(p.mode & MODE_DYNAMIC)) return static_key(p, c.x, c.y, c.z);                     // (w lane unused)
    // (the mode branch around the row's load, constant modes inside: the row stays one 16-byte load behind one branch)
    const uint32_t si = p.scene_idx[g];
    if (p.mode & MODE_INT) return dynamic_key(MODE_INT, scene_row(p.rows, MODE_INT, si), c.x, c.y, c.z, c.w);
    return dynamic_key(0u, scene_row(p.rows, 0u, si), c.x, c.y, c.z, c.w);
}

// The housekeeping folded into the first kernel of a sort (two launches and their boundaries saved per sort): the radix digit
// totals are zeroed before any histogram adds to them, and the OTHER SortFrame is reset for the next sort.  t / stride: the
// thread's index in the grid / the grid's size.  keep_slot: the slot of group rows this launch itself adds to (k_depth_key_hist) -
// left alone here, zeroed by the sort before (gs_sorter::clean_slot).
constexpr uint32_t RADIX_SLOT_WORDS = RADIX_MAX_GROUPS * RADIX_BINS;
__device__ __forceinline__ void sort_begin(const KeyParams& p, uint32_t t, uint32_t stride, uint32_t keep_slot = 0xFFFFFFFFu) {
    for (uint32_t w = t; w < (uint32_t)RADIX_TOTAL_WORDS; w += stride)
        if (w / RADIX_SLOT_WORDS != keep_slot) p.digit_total[w] = 0u;
    if (t < SORT_SHARDS) {
        p.next_frame->key_min[t] = KEY_MIN_INIT;
        p.next_frame->key_max[t] = KEY_MAX_INIT;
    }
    if (t == 0) {
        p.next_frame->clamped = 0;
        p.next_frame->kept = 0;
    }
}

// Min / max of the keys a thread has seen, and their way into the sort's SortFrame.
// No guard for a wave or workgroup that saw nothing: it publishes the two initial values, and an atomicMin with KEY_MIN_INIT
// (atomicMax with KEY_MAX_INIT) cannot change a word that started there - the same SortFrame with or without the test, and the
// streaming kernels do without the compare and branch.
struct MinMax {
    int32_t lo = KEY_MIN_INIT, hi = KEY_MAX_INIT;
    __device__ __forceinline__ void take(int32_t k) {
        lo = min(lo, k);
        hi = max(hi, k);
    }
    __device__ __forceinline__ void take(const int4& k) {
        lo = min(min(lo, k.x), min(min(k.y, k.z), k.w));
        hi = max(max(hi, k.x), max(max(k.y, k.z), k.w));
    }
    __device__ __forceinline__ void reduce_wave() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
    }
    // one device-scope word retires ~88 atomics per microsecond: 2 x 512 workgroups on one pair of words were ~10 us of
    // k_depth_key's tail.  SORT_SHARDS pairs, reduced by whoever reads them (SortFrame::lo() / hi()).
    __device__ __forceinline__ void publish(SortFrame* f, uint32_t shard) const {
        atomicMin(&f->key_min[shard % SORT_SHARDS], lo);
        atomicMax(&f->key_max[shard % SORT_SHARDS], hi);
    }
    // per wave (the whole wave calls)
    __device__ __forceinline__ void publish_wave(SortFrame* f, uint32_t shard) {
        reduce_wave();
        if ((threadIdx.x & 63u) == 0u) publish(f, shard);
    }
    // per workgroup of WAVES waves, through LDS (the whole workgroup calls).  Holds the workgroup's ONE barrier: what the kernel
    // staged in LDS before the call may be read after it.
    template <int WAVES>
    __device__ __forceinline__ void publish_block(SortFrame* f) {
        __shared__ int32_t s_lo[WAVES], s_hi[WAVES];
        reduce_wave();
        if ((threadIdx.x & 63u) == 0u) {
            s_lo[threadIdx.x >> 6] = lo;
            s_hi[threadIdx.x >> 6] = hi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            lo = s_lo[0];
            hi = s_hi[0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) {
                lo = min(lo, s_lo[w]);
                hi = max(hi, s_hi[w]);
            }
            publish(f, blockIdx.x);
        }
    }
};

// Phase A: keys for list positions [sort_start, render_count) + device-wide min / max.
// VEC4: identity index list + static integer mode (the Viewer's default, cull off): each lane reads 4 consecutive
// splats per plane as one 16-byte load and writes 4 keys as one 16-byte store.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_depth_key(KeyParams p) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (p.ext_minmax) {
        // visibility-culled sort: k_minmax_count did the housekeeping and took min / max over EVERY splat; this launch only
        // keys the compacted list, whose length lives on the device
        const uint32_t R = *p.count_dev;
        for (uint32_t i = t; i < R; i += stride) p.keys_out[i] = depth_key_one(p, min(p.idx_in[i], p.last_splat));
        return;
    }
    sort_begin(p, t, stride);
    MinMax mm;
    auto scalars = [&](uint32_t begin, uint32_t end) {     // identity-list positions [begin, end), one at a time
        for (uint32_t i = begin + t; i < end; i += stride) {
            const int32_t k = depth_key_one(p, i);
            p.keys_out[i] = k;
            mm.take(k);
        }
    };
    if (VEC4) {
        // positions [a4*4, b4*4) are handled as vectors, the ragged head/tail as scalars by the first lanes
        const uint32_t a4 = (p.sort_start + 3u) / 4u, b4 = p.render_count / 4u;
        const uint4* x4 = reinterpret_cast<const uint4*>(p.cx);
        const uint4* y4 = reinterpret_cast<const uint4*>(p.cy);
        const uint4* z4 = reinterpret_cast<const uint4*>(p.cz);
        int4* o4 = reinterpret_cast<int4*>(p.keys_out);
        for (uint32_t v = a4 + t; v < b4; v += stride) {
            const int4 k = static_key_int4(p, x4[v], y4[v], z4[v]);
            o4[v] = k;
            mm.take(k);
        }
        if (a4 <= b4) {
            const uint32_t head_end = min(a4 * 4u, p.render_count), tail_begin = max(b4 * 4u, head_end);
            scalars(p.sort_start, head_end);
            scalars(tail_begin, p.render_count);
        } else {                                           // fewer than one aligned vector: all scalar
            scalars(p.sort_start, p.render_count);
        }
    } else {
        // the list's length may live on the device (an asynchronous gs_tree_gather): the sorted result then has that length,
        // published where the consumers of a culled sort look for it
        const uint32_t R = p.count_dev ? min(*p.count_dev, p.render_count) : p.render_count;
        if (p.count_dev && t == 0) p.frame->kept = R;
        for (uint32_t i = p.sort_start + t; i < R; i += stride) {
            const uint32_t g = p.idx_in ? min(p.idx_in[i], p.last_splat) : i;
            const int32_t k = depth_key_one(p, g);
            p.keys_out[i] = k;
            mm.take(k);
        }
    }
    mm.publish_block<4>(p.frame);
}

// Phase A with the per-splat frustum cull (gs_sorter_set_frustum_cull).  Same keys, same min / max over EVERY list
// position (so the bucket of a kept splat is the one the full sort gives it), plus one keep bit per position:
//     q = mvp * (x, y, z, 1)    fp32, ((m0*x + m4*y) + m8*z) + m12 per row, no contraction
//     drop  <=>  |q.x| > 1.25*q.w + 0.01  or  |q.y| > 1.25*q.w + 0.01  or  q.z < -(1.01*q.w + 0.01)  or  q.z > 1.01*q.w + 0.01
// with (x, y, z) = the sorter's own centres as floats (integer mode: (float)int * 0.001f).  The vertex stage drops a
// splat on |clip.xy| > 1.2 w, clip.z < -1.2 w or ndc.z outside [-1, 1] (SplatMaterial.js:160-164 and the GL clip of a
// quad that sits at its centre's depth), so for the same camera the kept set is a superset of what can reach the
// frame, and the frame is bit-identical to the one the full sort produces.  Restated in oracle.frustum_keep.
__device__ __forceinline__ bool frustum_keep_one(const float* m, const float3 c) {
    float q[4];
#pragma unroll
    for (int r = 0; r < 4; r++)
        q[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[r], c.x), __fmul_rn(m[4 + r], c.y)), __fmul_rn(m[8 + r], c.z)), m[12 + r]);
    const float lim_xy = __fadd_rn(__fmul_rn(1.25f, q[3]), 0.01f);
    const float lim_z = __fadd_rn(__fmul_rn(1.01f, q[3]), 0.01f);
    return !(fabsf(q[0]) > lim_xy || fabsf(q[1]) > lim_xy || q[2] < -lim_z || q[2] > lim_z);
}

__device__ __forceinline__ bool frustum_keep_int(const float* m, uint32_t x, uint32_t y, uint32_t z) {
    return frustum_keep_one(m, centre_int_as_float(x, y, z));
}

// VEC4 (identity list, static integer mode): lane l of a wave owns positions 4*(v0 + l) .. +3 of a 256-position window,
// read as three 16-byte plane loads; the 4 keep bits of 16 neighbouring lanes are OR-combined into one mask word.
// Otherwise: 4 positions per lane, 64 apart, so 4 index loads and then 4 centre gathers are in flight per lane and
// every ballot is one mask word.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_depth_key_cull(KeyParams p) {
    const uint32_t stride = gridDim.x * blockDim.x;               // a multiple of 64
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    sort_begin(p, t, stride);
    MinMax mm;
    const uint32_t lane = threadIdx.x & 63;
    // sort_start == 0 in this variant; the length of a gathered list may live on the device (asynchronous gs_tree_gather)
    const uint32_t R = (!VEC4 && p.count_dev) ? min(*p.count_dev, p.render_count) : p.render_count;
    if (VEC4) {
        const uint32_t nvec = (R + 3u) / 4u, full = R / 4u, padded = (nvec + 63u) & ~63u;
        const uint4* x4 = reinterpret_cast<const uint4*>(p.cx);
        const uint4* y4 = reinterpret_cast<const uint4*>(p.cy);
        const uint4* z4 = reinterpret_cast<const uint4*>(p.cz);
        int4* o4 = reinterpret_cast<int4*>(p.keys_out);
        for (uint32_t v = t; v < padded; v += stride) {
            uint32_t nib = 0;
            if (v < full) {
                const uint4 x = x4[v], y = y4[v], z = z4[v];
                const int4 k = static_key_int4(p, x, y, z);
                o4[v] = k;
                mm.take(k);
                nib = (frustum_keep_int(p.mvp, x.x, y.x, z.x) ? 1u : 0u) | (frustum_keep_int(p.mvp, x.y, y.y, z.y) ? 2u : 0u) |
                      (frustum_keep_int(p.mvp, x.z, y.z, z.z) ? 4u : 0u) | (frustum_keep_int(p.mvp, x.w, y.w, z.w) ? 8u : 0u);
            } else if (v < nvec) {                                 // the ragged last vector
                for (uint32_t c = 0; c < 4u; c++) {
                    const uint32_t i = 4u * v + c;
                    if (i < R) {
                        const uint32_t x = p.cx[i], y = p.cy[i], z = p.cz[i];
                        const int32_t k = static_key_int(p, x, y, z);
                        p.keys_out[i] = k;
                        mm.take(k);
                        nib |= frustum_keep_int(p.mvp, x, y, z) ? (1u << c) : 0u;
                    }
                }
            }
            unsigned long long word = (unsigned long long)nib << (4u * (lane & 15u));
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) word |= __shfl_xor(word, o, 64);
            if ((lane & 15u) == 0u) p.keep[v >> 4] = word;          // positions 4v .. 4v+63
        }
    } else {
        const uint32_t padded = (R + 255u) & ~255u;
        for (uint32_t base = (t >> 6) * 256u; base < padded; base += (stride >> 6) * 256u) {
            uint32_t g[4];
            bool in[4], keep[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t i = base + 64u * k + lane;
                in[k] = i < R;
                g[k] = in[k] ? (p.idx_in ? min(p.idx_in[i], p.last_splat) : i) : 0u;
            }
            uint4 c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = in[k] ? p.aos[g[k]] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                keep[k] = false;
                if (in[k]) {
                    const uint32_t i = base + 64u * k + lane;
                    float3 centre;
                    const int32_t key = static_key_centre(p, c[k], centre);
                    p.keys_out[i] = key;
                    mm.take(key);
                    keep[k] = frustum_keep_one(p.mvp, centre);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned long long word = __ballot(keep[k]);
                if (lane == 0 && base + 64u * k < padded) p.keep[(base >> 6) + k] = word;
            }
        }
    }
    // (the number of kept positions is published by pass 0 of the radix sort - the sum of its digit totals - instead of by
    // one atomicAdd per workgroup on a single word here: radix.hpp, count_out)
    mm.publish_block<4>(p.frame);
}

// ---------------------------------------------------------------------------------------------------
// Octree-gathered lists (gs_tree_gather -> gs_sorter_sort_gathered): the copy and phase A in one kernel.
// gs_tree_gather only PLANS (per kept leaf: where its index list goes); a full sort of a static scene then runs this kernel
// instead of k_tree_copy + k_depth_key(_cull): one wave per leaf streams the leaf's indexes, its centres and its payloads from
// arrays kept in the TREE'S leaf-major order (leaf_centers / leaf_pos: built once per (tree, centres, bound mesh) by
// k_tree_leaf_cache), and writes the list, its payloads, its keys, min / max and - with the per-splat frustum cull - the keep
// bits.  Rounds 2-3 keyed the gathered list through 16-byte centre gathers at random (86 us for 4.4 M entries: MI355X retires
// ~55 G random accesses per second whatever their size, tools/probes/gather_rate.hip) and translated the payloads through
// another random gather in pass 0 of the radix sort.
struct TreeCopyParams {
    TreeGatherView v;
    const uint4* leaf_centers;
    const uint32_t* leaf_pos;
    uint32_t* idx_out;
    uint32_t* pay_out;
};

__global__ __launch_bounds__(256) void k_tree_leaf_cache(const uint32_t* __restrict__ leaf_indexes, uint32_t n, const uint4* __restrict__ caos,
                                                         const uint32_t* __restrict__ map, uint32_t last_splat,
                                                         uint4* __restrict__ leaf_centers, uint32_t* __restrict__ leaf_pos) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t o = min(leaf_indexes[j], last_splat);
        leaf_centers[j] = caos[o];
        leaf_pos[j] = map ? map[o] : o;
    }
}

template <bool CULL>
__global__ __launch_bounds__(256) void k_tree_copy_keys(TreeCopyParams c, KeyParams p) {
    const uint32_t stride = gridDim.x * blockDim.x, gt = blockIdx.x * blockDim.x + threadIdx.x;
    sort_begin(p, gt, stride);
    if (!CULL && gt == 0) p.frame->kept = c.v.totals[0];     // the list's length, where the consumers of a culled sort look for it
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    MinMax mm;
    // A wave's work is a sequence of ROUNDS: 256 consecutive entries (four 64-splat slices, twelve loads that leave together) of
    // one kept leaf's list - a leaf holds ~200 splats, so most leaves are one round.  Round 6: the loads of round k + 1 are issued
    // BEFORE round k is keyed and stored (two register sets, no copies: the loop is unrolled by two), also across leaves; before,
    // a wave's memory system idled between the stores of one leaf and the loads of the next (the same finding as k_cull_front,
    // load -> compute -> store in step leaves the memory idle between bursts).  The loads are unconditional - a lane
    // past the end of its leaf, or a wave past its last round, reads entry 0 of the round's leaf / of the arrays - because a load
    // inside a branch costs a full s_waitcnt at the join, taken or not.
    struct Round { uint32_t off, n, src, t0, valid; };
    struct Loads { uint32_t idx[4], pos[4]; uint4 ce[4]; };
    const uint32_t wstride = gridDim.x * 4u;
    uint32_t leaf = blockIdx.x * 4u + wave;                  // the next leaf whose header words are in m_*
    uint32_t m_off = 0xFFFFFFFFu, m_n = 0, m_src = 0;
    if (leaf < c.v.leaves) { m_off = c.v.leaf_offset[leaf]; m_n = c.v.leaf_count[leaf]; m_src = c.v.leaf_begin[leaf]; }
    auto advance = [&](Round& r) {                           // (wave-uniform)
        if (r.valid && r.t0 + 256u < r.n) { r.t0 += 256u; return; }
        r.valid = 0u;
        while (leaf < c.v.leaves) {
            const uint32_t off = m_off, n = m_n, src = m_src;
            leaf += wstride;
            if (leaf < c.v.leaves) { m_off = c.v.leaf_offset[leaf]; m_n = c.v.leaf_count[leaf]; m_src = c.v.leaf_begin[leaf]; }
            if (off != 0xFFFFFFFFu && n) { r.off = off; r.n = n; r.src = src; r.t0 = 0u; r.valid = 1u; return; }   // (else: a culled leaf)
        }
    };
    auto load = [&](const Round& r, Loads& L) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t t = r.t0 + 64u * k + lane;
            const uint32_t j = r.valid ? r.src + (t < r.n ? t : 0u) : 0u;
            L.idx[k] = c.v.leaf_indexes[j];
            L.pos[k] = c.leaf_pos[j];
            L.ce[k] = c.leaf_centers[j];
        }
    };
    unsigned long long carry = 0ull;                         // (lane 0) keep bits of this leaf that belong to the next round's first word
    auto process = [&](const Round& r, const Loads& L) {
        const uint32_t off = r.off, n = r.n, t0 = r.t0;
        if (t0 == 0u) carry = 0ull;
        unsigned long long bits[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t t = t0 + 64u * k + lane;
            const bool in = t < n;
            float3 centre;
            const int32_t key = static_key_centre(p, L.ce[k], centre);
            if (in) {
                c.idx_out[off + t] = L.idx[k];
                c.pay_out[off + t] = L.pos[k];
                p.keys_out[off + t] = key;
                mm.take(key);
            }
            if (CULL) bits[k] = __ballot(in && frustum_keep_one(p.mvp, centre));
        }
        if (CULL && lane == 0u) {
            // The round's 256 list positions start at `first`: four words of the (zeroed) keep mask and a carry into the
            // fifth, which the next round of this leaf completes.  A word that lies wholly inside this leaf's range is ours
            // alone - a plain store; the words the leaf shares with its neighbours in the list take an atomicOr (two per
            // slice, 136 k atomics per gather, were ~15 us of this kernel).
            const uint32_t first = off + t0, sh = first & 63u, w0 = first >> 6;
            unsigned long long W[4];
            W[0] = carry | (bits[0] << sh);
#pragma unroll
            for (int j = 1; j < 4; j++) W[j] = (bits[j] << sh) | (sh ? bits[j - 1] >> (64u - sh) : 0ull);
            carry = sh ? bits[3] >> (64u - sh) : 0ull;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t wbeg = (w0 + (uint32_t)j) * 64u;            // first list position of the word
                if (wbeg >= off && wbeg + 64u <= off + n) p.keep[w0 + j] = W[j];
                else if (W[j]) atomicOr(&p.keep[w0 + j], W[j]);
            }
            if (t0 + 256u >= n && carry) atomicOr(&p.keep[w0 + 4u], carry);   // the leaf's last round: its tail word
        }
    };
    Round ra = {0u, 0u, 0u, 0u, 0u}, rb;
    Loads A, B;
    advance(ra);
    load(ra, A);
    while (ra.valid) {
        rb = ra; advance(rb);
        load(rb, B);                                         // in flight while A is keyed and stored
        process(ra, A);
        if (!rb.valid) break;
        ra = rb; advance(ra);
        load(ra, A);
        process(rb, B);
    }
    mm.publish_block<4>(p.frame);                            // (CULL: the kept count is published by pass 0 of the radix sort, radix.hpp count_out)
}

// ---------------------------------------------------------------------------------------------------
// Visibility-culled sort (gs_sorter_set_visibility_cull): compact, then sort the survivors.
// The bound mesh's vertex stage left one bit per ORIGINAL splat index (gs_mesh::vis_orig) for this camera and strip.  The
// reference's buckets depend on min / max over every sorted position, so every splat is still keyed once - but nothing is
// stored for the ones that draw nothing:
//   k_minmax_count   one streaming pass over the centres (12 bytes per splat): min / max, and the number of set mask bits of
//                    every workgroup's contiguous chunk of positions;
//   k_mask_compact   mask -> ascending list of the surviving splat indexes (a subsequence of the identity list, so the stable
//                    sort keeps the reference's tie order), its length -> SortFrame::kept;
//   then the ordinary index-list sort runs on that list with the min / max above (k_depth_key ext_minmax, DepthLoader n_dev).
// A rank of a multi-GPU draw therefore streams 12 bytes per splat and radix-sorts only what its strip draws.
// (VC_THREADS = 256 threads, VC_SPAN = 1024 positions per workgroup iteration - 4 per lane, 32 mask words: sort_plan.hpp)

// DYN: a dynamic-mode sorter (a compile-time instance, as in k_cull_front) - the key of a position comes from five planes, x, y, z,
// w and the scene index (20 bytes per splat, one 16-byte vector per plane and lane in both modes), and the scene's row from LDS.
template <bool DYN>
__global__ __launch_bounds__(VC_THREADS) void k_minmax_count(KeyParams p, const uint32_t* __restrict__ mask, uint32_t chunk_len,
                                                             uint32_t* __restrict__ chunk_counts) {
    __shared__ uint32_t s_cnt[4];
    __shared__ uint4 s_rows[DYN ? GS_MAX_SCENES : 1];
    sort_begin(p, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (DYN) {
        stage_scene_rows(p, s_rows);
        __syncthreads();
    }
    const uint32_t N = p.render_count;
    const uint32_t begin = min(blockIdx.x * chunk_len, N), end = min(begin + chunk_len, N);     // chunk_len % VC_SPAN == 0
    MinMax mm;
    uint32_t cnt = 0;
    // DYN: the five vectors of span k + 1 are requested before span k is keyed (two register sets, as in k_cull_front: the grid is
    // two workgroups per CU, so what is in flight per lane is what hides the latency).  Unconditional loads, clamped into the list -
    // the planes are padded by 16 bytes, so the vector that holds the list's last position is readable whatever N is.
    struct Span { uint4 x, y, z, w, s; };
    Span cur, nxt;
    auto fetch = [&](uint32_t base, Span& v) {
        const uint32_t i0 = base + 4u * threadIdx.x, q = (i0 < N ? i0 : 0u) >> 2;
        v.x = reinterpret_cast<const uint4*>(p.cx)[q]; v.y = reinterpret_cast<const uint4*>(p.cy)[q];
        v.z = reinterpret_cast<const uint4*>(p.cz)[q]; v.w = reinterpret_cast<const uint4*>(p.cw)[q];
        v.s = reinterpret_cast<const uint4*>(p.scene_idx)[q];
    };
    if constexpr (DYN) { if (begin < end) fetch(begin, cur); }
    for (uint32_t base = begin; base < end; base += VC_SPAN) {
        const uint32_t i0 = base + 4u * threadIdx.x;
        if constexpr (DYN) {
            fetch(base + VC_SPAN, nxt);
            const int4 k = dynamic_key4(p.mode, s_rows, cur.x, cur.y, cur.z, cur.w, cur.s);
            if (i0 + 4u <= end) {
                mm.take(k);
            } else {                                               // (the list's ragged end: min / max over its positions only)
                if (i0 < end) mm.take(k.x);
                if (i0 + 1u < end) mm.take(k.y);
                if (i0 + 2u < end) mm.take(k.z);
            }
            cur = nxt;
        } else if ((p.mode & MODE_INT) && i0 + 4u <= end) {        // 16-byte plane loads
            mm.take(static_key_int4(p, reinterpret_cast<const uint4*>(p.cx)[i0 >> 2], reinterpret_cast<const uint4*>(p.cy)[i0 >> 2],
                                    reinterpret_cast<const uint4*>(p.cz)[i0 >> 2]));
        } else {
            for (uint32_t i = i0; i < min(i0 + 4u, end); i++) mm.take(static_key_planes(p, i));
        }
        const uint32_t w = (base >> 5) + threadIdx.x;              // the 32 mask words of this span
        // (a sort over fewer splats than the vertex stage looked at leaves set bits beyond `end` in the last word)
        if (threadIdx.x < VC_SPAN / 32u && (w << 5) < end)
            cnt += (uint32_t)__popc(mask[w] & (end - (w << 5) >= 32u ? 0xFFFFFFFFu : (1u << (end - (w << 5))) - 1u));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = cnt;
    mm.publish_block<4>(p.frame);                                  // (and its barrier: s_cnt is complete)
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// The mask is CONSUMED: every word is copied to the sorter's own buffer (gs_sorter_debug_read) and zeroed, which is the state the
// next gs_mesh_project expects (its survivors set bits with atomicOr) - a 725 KB memset per frame less on every rank.
__global__ __launch_bounds__(VC_THREADS) void k_mask_compact(uint32_t* __restrict__ mask, uint32_t* __restrict__ mask_copy,
                                                             const uint32_t* __restrict__ chunk_counts,
                                                             uint32_t N, uint32_t chunk_len, uint32_t* __restrict__ idx_out,
                                                             SortFrame* __restrict__ frame) {
    __shared__ uint32_t s_tmp[4], s_before[4], s_all[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t before = 0, all = 0;                                   // survivors of the chunks before this one / of all chunks
    for (uint32_t c = threadIdx.x; c < gridDim.x; c += VC_THREADS) {
        const uint32_t v = chunk_counts[c];
        all += v;
        before += c < blockIdx.x ? v : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o, 64);
        all += __shfl_xor(all, o, 64);
    }
    if (lane == 0u) { s_before[wave] = before; s_all[wave] = all; }
    __syncthreads();
    uint32_t out = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) frame->kept = s_all[0] + s_all[1] + s_all[2] + s_all[3];
    const uint32_t begin = min(blockIdx.x * chunk_len, N), end = min(begin + chunk_len, N);
    for (uint32_t base = begin; base < end; base += 32u * VC_THREADS) {        // one mask word (32 positions) per thread
        const uint32_t first = base + 32u * threadIdx.x;
        uint32_t w = 0u;
        if (first < end) {
            w = mask[first >> 5];
            mask_copy[first >> 5] = w;
            if (w) mask[first >> 5] = 0u;
            if (end - first < 32u) w &= (1u << (end - first)) - 1u;        // positions beyond this sort's list
        }
        uint32_t total;
        uint32_t o = out + block_excl_scan<4>((uint32_t)__popc(w), s_tmp, &total);
        while (w) {
            idx_out[o++] = first + (uint32_t)__builtin_ctz(w);
            w &= w - 1u;
        }
        out += total;
    }
}

// Round 5: the same front end as TWO kernels that never gather.  Round 4's chain keyed the survivors through one 16-byte centre
// gather each (k_depth_key over the compacted list: 1.44 M gathers at the machine's ~55 G/s = 26 us for a full frame) and
// translated their payloads through another gather in pass 0; but the survivors are a SUBSEQUENCE of the identity list, so the
// pass that streams every centre for min / max can key them on the way:
//   k_mask_count   survivors per chunk of positions, from the mask alone (1 bit per splat: 0.7 MB) + the sort's housekeeping;
//   k_cull_front   one streaming pass over the centres (12 bytes per splat): min / max over EVERY splat, and for the survivors of
//                  the chunk - whose first output slot is the sum of the earlier chunks' counts - key and payload (the bound
//                  mesh's position, read for survivors only) written to the compacted list.  The mask is consumed as before.
// No look-back, no spinning: the offsets come from the first kernel's counts.
// A workgroup owns a contiguous run of positions (chunk_len % VC_TURN == 0) and walks it in turns of VC_TURN: wave w of the workgroup
// takes VC_UNROLL consecutive spans of the turn, a lane four consecutive positions of a span (one 16-byte load per
// plane), so the workgroup streams 8 KB per plane per turn and the chip ~2000 streams in all.  A wave's first output slot in a
// turn = the workgroup's running offset + the survivors of the lower waves in this turn (one barrier per turn, counts double
// buffered); inside a wave the prefix over the 64 lanes is a DPP scan.  (Turn = 2048 positions with VC_UNROLL = 2.)
// (History, r05c-h: cutting the list per workgroup with a block scan every 1024 positions cost a rank's strip 22 barriers per chunk
// for nothing; one contiguous run per WAVE needs no barrier at all but makes 8192 concurrent DRAM streams - 36-42 us for the 93 MB;
// spans handled one by one put a store round trip between them - predicated stores cannot be counted, the compiler drains the queue -
// and a run-time `map ? load : index` put every payload load in a branch of its own with a full wait behind it.)
// (VC_WAVE_SPAN, VC_UNROLL and VC_TURN = 2048 positions per workgroup and turn: sort_plan.hpp)

__global__ __launch_bounds__(VC_THREADS) void k_mask_count(KeyParams p, const uint32_t* __restrict__ mask, uint32_t chunk_len,
                                                           uint32_t* __restrict__ chunk_counts) {
    __shared__ uint32_t s_cnt[4];
    sort_begin(p, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    const uint32_t N = p.render_count;
    const uint32_t begin = min(blockIdx.x * chunk_len, N), end = min(begin + chunk_len, N);
    uint32_t cnt = 0;
    for (uint32_t first = begin + 32u * threadIdx.x; first < end; first += 32u * VC_THREADS) {
        uint32_t w = mask[first >> 5];
        if (end - first < 32u) w &= (1u << (end - first)) - 1u;            // positions beyond this sort's list
        cnt += (uint32_t)__popc(w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// k_mask_count for a projection whose by-original-index mask was NOT written by the vertex stage (round 6).  gs_mesh_project used
// to set one bit per survivor with an atomicOr at inv_perm[position]: 1.44 M atomics scattered over a 0.7 MB table cost k_project
// 25 us of a full C3 frame (47 -> 72 us in the kernel table of the visibility-culled frame, profiles/r06n_vis_n1_kstats.txt).
// The sorter can build the same mask from what it streams anyway: position i of the identity list is the splat at storage
// position map[i], whose bit is in the vertex stage's own storage-order mask (vis_mask, 1 bit per position, 0.7 MB: it stays in
// L2) - and three of four splats sit in a storage block with no survivor at all (block_any, kept as bits in LDS as the binner
// does), so only a quarter of the positions gather anything.  64 positions per wave and step (ballot -> one 8-byte word), four
// steps in flight.  Writes the mask words of its chunk (so k_cull_front / k_mask_compact find what they always found) and the
// chunk's survivor count; full-frame projections only - a strip keeps a few per cent and pays few atomics.
constexpr uint32_t VC_ANY_WORDS = 2048;                    // block_any as bits in LDS: 65536 storage blocks = 16.7 M splats
__global__ __launch_bounds__(VC_THREADS) void k_mask_derive_count(KeyParams p, const uint32_t* __restrict__ map,
                                                                  const unsigned long long* __restrict__ vis_mask,
                                                                  const uint8_t* __restrict__ block_any, uint32_t blocks, uint32_t chunk_len,
                                                                  uint32_t subs, unsigned long long* __restrict__ mask64,
                                                                  uint32_t* __restrict__ chunk_counts) {
    __shared__ uint32_t s_cnt[4];
    __shared__ uint32_t s_any[VC_ANY_WORDS];
    sort_begin(p, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    const bool coarse = blocks <= VC_ANY_WORDS * 32u;
    if (coarse) {
        for (uint32_t w = threadIdx.x; w < (blocks + 31u) / 32u; w += VC_THREADS) {
            const uint4* src = reinterpret_cast<const uint4*>(block_any + 32u * w);               // (the buffer is padded to 64 bytes)
            const uint4 a = src[0], b = src[1];
            const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 8; k++)
                bits |= (((v[k] & 0xFFu) ? 1u : 0u) | ((v[k] & 0xFF00u) ? 2u : 0u) | ((v[k] & 0xFF0000u) ? 4u : 0u) |
                         ((v[k] & 0xFF000000u) ? 8u : 0u)) << (4 * k);
            s_any[w] = bits;
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t N = p.render_count;
    // `subs` workgroups share a chunk of the front end (which runs two workgroups per CU; this kernel is a chain of two dependent
    // round trips per round - the map, then the gather - and wants every SIMD full of waves): piece blockIdx.x % subs of chunk
    // blockIdx.x / subs, counts per piece.  A wave takes DERIVE_STEPS x 64 consecutive positions per round, and the NEXT round's
    // map words are fetched before this round's gathers are used.  (One workgroup per chunk, 4 steps, no prefetch: 25 us for the
    // C3 frame's 5.8 M positions; 8 steps + prefetch: 20.9 us; r06p kernel tables.)
    const uint32_t chunk = blockIdx.x / subs, piece = blockIdx.x % subs, piece_len = chunk_len / subs;     // chunk_len % (4096 * subs) == 0
    const uint32_t cend = min(min(chunk * chunk_len, N) + chunk_len, N);
    const uint32_t begin = min(chunk * chunk_len + piece * piece_len, cend), end = min(begin + piece_len, cend);
    uint32_t cnt = 0;
    constexpr uint32_t DERIVE_STEPS = 8, DERIVE_ROUND = DERIVE_STEPS * 64u * (VC_THREADS / 64u);
    static_assert(VC_TURN % DERIVE_ROUND == 0, "a chunk is a whole number of rounds");
    uint32_t nxt[DERIVE_STEPS];
    auto fetch = [&](uint32_t base) {
#pragma unroll
        for (uint32_t k = 0; k < DERIVE_STEPS; k++) nxt[k] = map[min(base + 64u * k + lane, N - 1u)];     // (unconditional, clamped)
    };
    if (begin < end) fetch(begin + DERIVE_STEPS * 64u * wave);
    for (uint32_t base = begin + DERIVE_STEPS * 64u * wave; base < end; base += DERIVE_ROUND) {
        uint32_t pos[DERIVE_STEPS];
        bool live[DERIVE_STEPS];
#pragma unroll
        for (uint32_t k = 0; k < DERIVE_STEPS; k++) {
            pos[k] = nxt[k];
            live[k] = base + 64u * k + lane < end;
        }
        fetch(min(base + DERIVE_ROUND, N - 1u));
#pragma unroll
        for (uint32_t k = 0; k < DERIVE_STEPS; k++)
            live[k] = live[k] && (coarse ? ((s_any[pos[k] >> 13] >> ((pos[k] >> 8) & 31u)) & 1u) != 0u : block_any[pos[k] >> 8] != 0);
        unsigned long long w[DERIVE_STEPS];
#pragma unroll
        for (uint32_t k = 0; k < DERIVE_STEPS; k++) w[k] = vis_mask[live[k] ? pos[k] >> 6 : 0u];         // (unconditional: no wait at a join)
#pragma unroll
        for (uint32_t k = 0; k < DERIVE_STEPS; k++) {
            const unsigned long long word = __ballot(live[k] && ((w[k] >> (pos[k] & 63u)) & 1ull));
            cnt += (uint32_t)__popcll(word);                                                      // (the same value in every lane)
            if (lane == 0u && base + 64u * k < end) mask64[(base + 64u * k) >> 6] = word;
        }
    }
    if (lane == 0u) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// MAP: payloads come from the bound mesh's position table (a compile-time switch, see above)
// DYN: a dynamic-mode sorter - two more 16-byte vectors per lane and span (four w, four scene indexes: 24 bytes per position with
// the payload map instead of 16) and the scenes' rows of the mode in use from LDS, staged once per workgroup behind the barrier the
// prologue has anyway.  A compile-time instance for the reason MAP is one; every lane reads the row of each of its positions (no
// wave-uniform shortcut: scenes drawn at random per splat are as valid as scenes back to back).
struct CullTurnStatic {};
struct CullTurnDynamic { uint4 W[VC_UNROLL], S[VC_UNROLL]; };
template <bool MAP, bool DYN>
__global__ __launch_bounds__(VC_THREADS) void k_cull_front(KeyParams p, uint32_t* __restrict__ mask, uint32_t* __restrict__ mask_copy,
                                                           const uint32_t* __restrict__ chunk_counts, uint32_t chunk_len,
                                                           const uint32_t* __restrict__ map, uint32_t* __restrict__ pay_out, uint32_t subs) {
    __shared__ uint32_t s_before[4], s_all[4], s_turn[2][4];
    __shared__ uint4 s_rows[DYN ? GS_MAX_SCENES : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    static_assert(VC_THREADS == 256, "four waves per workgroup");
    if (DYN) stage_scene_rows(p, s_rows);                           // (published by the barrier below)
    uint32_t before = 0, all = 0;                                   // survivors of the chunks before this one / of all chunks
    // (the counts arrive in `subs` consecutive pieces per chunk: k_mask_count writes one, k_mask_derive_count one per sub-workgroup)
    const uint32_t pieces = gridDim.x * subs, mine = blockIdx.x * subs;
    for (uint32_t c0 = 0; c0 < pieces; c0 += 4u * VC_THREADS) {     // (four loads in flight per lane)
        uint32_t x[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) x[k] = chunk_counts[min(c0 + VC_THREADS * k + threadIdx.x, pieces - 1u)];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t c = c0 + VC_THREADS * k + threadIdx.x;
            all += c < pieces ? x[k] : 0u;
            before += c < mine ? x[k] : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o, 64);
        all += __shfl_xor(all, o, 64);
    }
    if (lane == 0u) { s_before[wave] = before; s_all[wave] = all; }
    __syncthreads();
    uint32_t out = s_before[0] + s_before[1] + s_before[2] + s_before[3];          // the workgroup's running output slot
    if (blockIdx.x == 0u && threadIdx.x == 0u) p.frame->kept = s_all[0] + s_all[1] + s_all[2] + s_all[3];
    const uint32_t N = p.render_count;
    const uint32_t begin = min(blockIdx.x * chunk_len, N), end = min(begin + chunk_len, N);       // chunk_len % VC_TURN == 0
    MinMax mm;
    const uint4* __restrict__ x4 = reinterpret_cast<const uint4*>(p.cx);
    const uint4* __restrict__ y4 = reinterpret_cast<const uint4*>(p.cy);
    const uint4* __restrict__ z4 = reinterpret_cast<const uint4*>(p.cz);
    const uint4* __restrict__ w4 = reinterpret_cast<const uint4*>(p.cw);
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(p.scene_idx);
    int32_t* __restrict__ keys_out = p.keys_out;
    const uint4* __restrict__ map4 = reinterpret_cast<const uint4*>(map);
    // The loads of turn t + 1 are issued BEFORE turn t is keyed and stored (two register sets): all workgroups run in step, so a
    // turn that loads, then computes, then stores left the memory system idle between the bursts - 36-44 us for 93 MB (r05h/i).
    struct Turn : std::conditional<DYN, CullTurnDynamic, CullTurnStatic>::type {
        uint4 X[VC_UNROLL], Y[VC_UNROLL], Z[VC_UNROLL], M[VC_UNROLL]; uint32_t raw[VC_UNROLL];
    };
    auto fetch = [&](uint32_t base, Turn& t) {
        const uint32_t wbase = base + wave * (VC_UNROLL * VC_WAVE_SPAN);    // this wave's spans of the turn
#pragma unroll
        for (uint32_t u = 0; u < VC_UNROLL; u++) {
            const uint32_t i0 = wbase + u * VC_WAVE_SPAN + 4u * lane;      // this lane's four positions of span u
            // (unconditional loads; the planes and the mesh's position table are padded by 16 bytes, so the vector that holds the
            // list's last position is readable whatever N is)
            const uint32_t ic = i0 < N ? i0 : 0u;
            t.X[u] = x4[ic >> 2]; t.Y[u] = y4[ic >> 2]; t.Z[u] = z4[ic >> 2];
            if constexpr (DYN) { t.W[u] = w4[ic >> 2]; t.S[u] = s4[ic >> 2]; }     // (padded as the other planes are)
            t.M[u] = MAP ? map4[ic >> 2] : make_uint4(ic, ic + 1u, ic + 2u, ic + 3u);   // the payloads travel with the centres
            t.raw[u] = i0 < end ? mask[i0 >> 5] : 0u;                      // the mask word of the four positions (eight lanes share one)
        }
    };
    Turn cur, nxt;
    if (begin < end) fetch(begin, cur);
    uint32_t turn = 0;
    for (uint32_t base = begin; base < end; base += VC_TURN, turn++) {
        const uint32_t wbase = base + wave * (VC_UNROLL * VC_WAVE_SPAN);
        fetch(min(base + VC_TURN, end - 1u), nxt);                          // (past the end: a clamped re-read, never used)
        // phase 1, registers only: keys, survivor nibbles and slots (relative to the wave's first) of all the spans of the turn ...
        int32_t K[VC_UNROLL][4];
        uint32_t nibs[VC_UNROLL], first[VC_UNROLL], mine_total = 0;
#pragma unroll
        for (uint32_t u = 0; u < VC_UNROLL; u++) {
            const uint32_t i0 = wbase + u * VC_WAVE_SPAN + 4u * lane;
            int32_t k[4] = {0, 0, 0, 0};
            uint32_t word = cur.raw[u];
            if (i0 < end && end - (i0 & ~31u) < 32u) word &= (1u << (end - (i0 & ~31u))) - 1u;    // positions beyond this sort's list
            if constexpr (DYN) {   // (the rows: unconditional LDS reads, the index masked into the table)
                const int4 k4 = dynamic_key4(p.mode, s_rows, cur.X[u], cur.Y[u], cur.Z[u], cur.W[u], cur.S[u]);
                k[0] = k4.x; k[1] = k4.y; k[2] = k4.z; k[3] = k4.w;
#pragma unroll
                for (uint32_t c = 0; c < 4u; c++)
                    if (i0 + c < end) mm.take(k[c]);
            } else {   // keys from the vectors (no memory access in this phase: a load in a branch here puts a full wait at its join)
                const uint32_t xs[4] = {cur.X[u].x, cur.X[u].y, cur.X[u].z, cur.X[u].w}, ys[4] = {cur.Y[u].x, cur.Y[u].y, cur.Y[u].z, cur.Y[u].w},
                               zs[4] = {cur.Z[u].x, cur.Z[u].y, cur.Z[u].z, cur.Z[u].w};
#pragma unroll
                for (uint32_t c = 0; c < 4u; c++) {
                    k[c] = static_key(p, xs[c], ys[c], zs[c]);
                    if (i0 + c < end) mm.take(k[c]);                       // (min / max over the list's positions only)
                }
            }
            const uint32_t nib = (word >> (i0 & 31u)) & 15u, mine = (uint32_t)__popc(nib);
            const uint32_t incl = wave_incl_scan_dpp(mine);
            nibs[u] = nib;
            first[u] = mine_total + incl - mine;
            mine_total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
#pragma unroll
            for (uint32_t c = 0; c < 4u; c++) K[u][c] = k[c];
        }
        // the wave's first slot of the turn: the survivors of the lower waves (counts double buffered: one barrier per turn)
        if (lane == 0u) s_turn[turn & 1u][wave] = mine_total;
        __syncthreads();
        uint32_t wave_out = out, turn_total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            const uint32_t c = s_turn[turn & 1u][w];
            wave_out += w < wave ? c : 0u;
            turn_total += c;
        }
        out += turn_total;
        // ... phase 2, every store of the turn behind them
#pragma unroll
        for (uint32_t u = 0; u < VC_UNROLL; u++) {
            const uint32_t i0 = wbase + u * VC_WAVE_SPAN + 4u * lane;
            // the mask is consumed: copied for gs_sorter_debug_read, then zeroed (no other wave touches these words, and this
            // wave has read them all)
            if (i0 < end && (i0 & 31u) == 0u) {
                mask_copy[i0 >> 5] = cur.raw[u];
                if (cur.raw[u]) mask[i0 >> 5] = 0u;
            }
            uint32_t o = wave_out + first[u];
            const uint32_t pm[4] = {cur.M[u].x, cur.M[u].y, cur.M[u].z, cur.M[u].w};
#pragma unroll
            for (uint32_t c = 0; c < 4u; c++)
                if ((nibs[u] >> c) & 1u) {                                 // (stores only: see phase 1)
                    keys_out[o] = K[u][c];
                    pay_out[o] = pm[c];
                    o++;
                }
        }
        cur = nxt;
    }
    mm.publish_wave(p.frame, blockIdx.x * 4u + wave);
}

// Phase B as a radix loader.  Logical element j <-> list position i = R-1-j (reverse traversal makes the
// stable ascending sort of key' = range-1-bucket equal to the reference's descending, tie-reversed order).
// IDX: the list is an index (or ready-made payload) array, not the identity - a compile-time switch: as a run-time `idx ? load : i`
// every index load sat in a branch of its own with a full memory wait behind it, eight serialised round trips per tile in every
// sort of a gathered / compacted list (r05k ISA of the pass-0 scatter).
struct DepthLoaderArgs {                   // what every (CULL, IDX) variant is built from; the kernel-argument layout of all of them
    const int32_t* __restrict__ keys;
    const unsigned long long* __restrict__ keep;   // CULL: 1 bit per list position (k_depth_key_cull)
    const uint32_t* __restrict__ idx;      // nullable: identity
    const uint32_t* __restrict__ map;      // nullable: payload = map[splat index] (a bound mesh's internal position)
    SortFrame* frame;
    const uint32_t* n_dev;                 // nullable: the list length lives on the device (visibility-culled sort)
    uint32_t sort_start, render_count, range;
    uint32_t last_splat;                   // list entries are clamped to it
    uint32_t count_clamps;                 // only the histogram launch counts, so each element counts once
    int32_t lo;
    float range_map;
    const uint16_t* __restrict__ keys16;   // NARROW: the radix key of every list position, as k_depth_key_hist<true> left it
};
// NARROW: the front end knew the key range and stored key' = range - 1 - bucket itself, 2 bytes per list position, instead of the
// depth: the loader reads that and decodes nothing (no range, no SortFrame, no bucket arithmetic between the scatter's two waits).
template <bool CULL, bool IDX, bool NARROW = false>
struct DepthLoaderT : DepthLoaderArgs {
    __device__ __forceinline__ void prepare() {
        if (NARROW) return;                                     // (a known-range sort: the list's length is on the host)
        if (n_dev) render_count = *n_dev;                       // sort_start is 0 in that variant
        // the sort's min / max live in SORT_SHARDS words each: lane l reads shard l, five xor-shuffles reduce them
        // (every thread reading all 64 words cost the histogram kernel 5 us)
        const uint32_t l = threadIdx.x & (SORT_SHARDS - 1u);
        set_range(frame->key_min[l], frame->key_max[l]);
    }
    // lo / hi: shard (lane % SORT_SHARDS) of the sort's min / max, as this lane read it
    __device__ __forceinline__ void set_range(int32_t lo_shard, int32_t hi) {
        lo = lo_shard;
#pragma unroll
        for (int o = SORT_SHARDS / 2; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        set_known_range(lo, hi);
        // wave-uniform by construction: keep both in scalar registers
        lo = __builtin_amdgcn_readfirstlane(lo);
        range_map = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(range_map)));
    }
    // the sort's min and max themselves (k_depth_key_hist has them as kernel arguments)
    __device__ __forceinline__ void set_known_range(int32_t key_lo, int32_t key_hi) {
        lo = key_lo;
        // sorter.cpp:142-143: (float)(range-1) / ((float)max - (float)min), fp32, correctly rounded
        range_map = __fdiv_rn((float)(range - 1), __fsub_rn((float)key_hi, (float)key_lo));
    }
    __device__ __forceinline__ uint32_t count() const { return render_count - sort_start; }
    __device__ __forceinline__ uint32_t bucket(uint32_t i) const { return bucket_of<false>(keys[i]); }
    // sorter.cpp:146: (int)((float)(mapped - min) * rangeMap): int32 wrap, one fp32 multiply, truncation.  Branch-free (selects):
    // the scatter decodes eight of these per lane between two waits.  COUNT: the histogram launch counts the clamped ones.
    template <bool COUNT>
    __device__ __forceinline__ uint32_t bucket_of(int32_t depth) const {
        const int32_t diff = (int32_t)((uint32_t)depth - (uint32_t)lo);
        const float f = __fmul_rn((float)diff, range_map);
        const bool fits = f >= -2147483648.0f && f < 2147483648.0f;   // else NaN (hi==lo) / overflow: WASM -> bucket 0
        const int32_t b = fits ? (int32_t)f : 0;
        const bool under = b < 0, over = !under && (uint32_t)b >= range;
        if (COUNT && count_clamps && (under || over)) atomicAdd(&frame->clamped, 1u);
        return under ? 0u : (over ? range - 1u : (uint32_t)b);
    }
    __device__ __forceinline__ uint32_t key(uint32_t j) const { return (range - 1) - bucket(render_count - 1 - j); }
    __device__ __forceinline__ uint32_t payload(uint32_t i) const {
        const uint32_t o = IDX ? min(ld32(idx, i), last_splat) : i;
        return map ? ld32(map, o) : o;
    }
    __device__ __forceinline__ uint32_t val(uint32_t j) const { return payload(render_count - 1 - j); }
    // pre + fetch = the memory reads of element j (the index list first, then everything that depends on it, so that a tile's
    // loads leave as two batches), decode = the arithmetic on them
    struct Raw { int32_t depth; uint32_t payload; };
    static __device__ __forceinline__ int prof_slot(int) { return 0; }       // GS_RADIX_PROFILE
    __device__ __forceinline__ uint32_t pre(uint32_t j) const {
        const uint32_t i = render_count - 1 - j;
        return IDX ? min(ld32(idx, i), last_splat) : i;
    }
    __device__ __forceinline__ Raw fetch(uint32_t j, uint32_t o) const {
        Raw r;
        r.depth = NARROW ? (int32_t)ld32(keys16, render_count - 1 - j) : ld32(keys, render_count - 1 - j);
        r.payload = map ? ld32(map, o) : o;
        return r;
    }
    __device__ __forceinline__ void decode(const Raw& r, uint32_t& k, uint32_t& v) const {
        k = NARROW ? (uint32_t)r.depth : (range - 1) - bucket_of<false>(r.depth);
        v = r.payload;
    }
    // the histogram's view of element j (NARROW: never launched - the front end left pass 0's rows - but the pass templates name it)
    typedef int32_t HRaw;
    __device__ __forceinline__ HRaw hist_fetch(uint32_t j) const {
        return NARROW ? (int32_t)ld32(keys16, render_count - 1 - j) : ld32(keys, render_count - 1 - j);
    }
    __device__ __forceinline__ uint32_t hist_key(HRaw depth) const { return NARROW ? (uint32_t)depth : (range - 1) - bucket_of<true>(depth); }
    __device__ __forceinline__ bool valid(uint32_t j) const {
        if (!CULL) return true;
        const uint32_t i = render_count - 1 - j;
        return (ld32(keep, i >> 6) >> (i & 63u)) & 1ull;
    }
};
typedef DepthLoaderT<false, false> DepthLoader;          // (the identity list without a cull: what k_debug_buckets walks)

// A pass that follows a PACKING pass (radix.hpp, PACK_OUT) reads ONE word per element: what is left of the key above a value of
// `val_bits` bits; its digit is the low byte of that remainder (shift 0), its histogram is ArrayLoader<uint32_t>'s over the same
// words with shift = val_bits.
struct PackedLoader {
    const uint32_t* __restrict__ words;
    const uint32_t* __restrict__ n_dev;   // device-resident count (nullable)
    uint32_t n_host, val_bits;
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ uint32_t count() const { return n_dev ? *n_dev : n_host; }
    struct Raw { uint32_t w; };
    __device__ __forceinline__ uint32_t pre(uint32_t) const { return 0u; }
    __device__ __forceinline__ Raw fetch(uint32_t j, uint32_t) const { return Raw{ld32(words, j)}; }
    __device__ __forceinline__ void decode(const Raw& r, uint32_t& k, uint32_t& v) const {
        k = r.w >> val_bits;
        v = r.w & ((1u << val_bits) - 1u);
    }
    __device__ __forceinline__ bool valid(uint32_t) const { return true; }
    static __device__ __forceinline__ int prof_slot(int) { return 1; }       // GS_RADIX_PROFILE
};

__global__ void k_copy_head(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ map, uint32_t* __restrict__ out,
                            uint32_t n, uint32_t last_splat) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t o = idx ? min(idx[i], last_splat) : i;
        out[i] = map ? map[o] : o;
    }
}

// (positions beyond a culled / gathered result's length hold stale words: clamped, so a caller that reads too far gets
// garbage indexes, never a fault)
__global__ void k_unmap(const uint32_t* __restrict__ in, const uint32_t* __restrict__ unmap, uint32_t* __restrict__ out,
                        uint32_t n, uint32_t last) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = unmap[min(in[i], last)];
}

// Phase A + the histogram of pass 0 in ONE streaming launch, for a sort whose exact key range the host already knows: a full sort
// of the identity list in static integer mode whose keys cannot wrap (sort_plan.cpp; gs_key_range: min / max of im . c over the extreme set of
// the centres, extreme_set.hpp).  A key's bucket needs the min and max over ALL keys (sorter.cpp:142-146); here they are kernel
// arguments, so a workgroup buckets and counts its keys as it makes them: no min / max reduction, no wait for another workgroup,
// no k_radix_hist and no re-read of the keys.  The grid is pass 0's scatter grid and a workgroup keys ITS chunk of that pass
// (radix_chunk; logical element j = list position R - 1 - j), tile after tile, so row ch.id and the group rows are what the scatter
// expects - also for lists too long for the chunk-staged scatter, where pass 0 runs the tile kernel over longer chunks.
// The range goes into every shard of the sort's SortFrame with plain stores: DepthLoader::prepare of the scatter, k_debug_buckets
// and the statistics read it as ever.  The group rows of pass 0 (`group_rows`, slot keep_slot) are added to inside this launch, so
// sort_begin leaves them alone: they were zeroed by the sort before (gs_sorter::clean_slot).
// NARROW (buckets of <= 16 bits): the kernel knows every key's final bucket as it makes it, so it stores the radix key itself,
// key' = range - 1 - bucket, as 16 bits at the key's list position - what it counts - and nothing goes to keys_out: 2 bytes per
// splat written here and 2 read by pass 0 (DepthLoaderT<.., .., true>) instead of 4 and 4, and no bucket arithmetic in the scatter.
// A lane owns TWO adjacent vectors per plane there and stores its eight keys as one 16-byte store, one such pair in flight
// (GS_KEY_HIST_PAIR = 2: two pairs; 0: one vector per lane and step as below, four keys as an 8-byte store - both measured slower,
// profiles/r08_narrow_keys_ab.txt).  gs_sorter::keys is stale after such a sort (sorter_refresh_keys).
// COMPACT (NARROW only): the centres come from the sorter's 16-bit offset planes (gs_sorter::cx16 ..: d = c - o per axis, o the
// per-axis minimum, every d in [0, 65535] - counted by the builder, k_compact_centres), 6 bytes per splat instead of 12.  The key is
// a wrapping 32-bit dot product, linear mod 2^32: im . c == im . o + im . d bit for bit, whatever wraps on the way; k0 = im . o is the
// host's.  One 16-byte vector per plane is a lane's eight positions, so three 16-byte loads feed the one 16-byte store, and
// GS_KEY_HIST_C16_UNITS of them are in flight per lane (one: 2 and 4 measured slower, profiles/r09_compact_centres_ab.txt).  The
// ragged head and tail read the same planes one position at a time.  Keys, buckets, counts and the stored bytes are those of the
// int32 planes.
constexpr uint32_t KEY_HIST_VECS = 3;      // 16-byte vectors per plane a thread has in flight (one chunk of the chunk-staged pass)
#ifndef GS_KEY_HIST_PAIR
#define GS_KEY_HIST_PAIR 1
#endif
#ifndef GS_KEY_HIST_C16_UNITS
#define GS_KEY_HIST_C16_UNITS 1
#endif
struct CompactCentres {                    // the 16-bit offset planes as k_depth_key_hist<true, true> reads them
    const uint16_t *x, *y, *z;
    uint32_t k0;                           // static_key_int of the offset itself, wrapping
};
// The static integer key of one position of those planes (dx, dy, dz < 2^16): uint32 wrap-around, as static_key_int's.
__device__ __forceinline__ int32_t compact_key_int(const KeyParams& p, uint32_t k0, uint32_t dx, uint32_t dy, uint32_t dz) {
    return (int32_t)(k0 + dx * (uint32_t)p.im0 + dy * (uint32_t)p.im1 + dz * (uint32_t)p.im2);
}
template <bool NARROW, bool COMPACT = false>
__global__ __launch_bounds__(HIST_THREADS) void k_depth_key_hist(KeyParams p, DepthLoader ld, int32_t key_lo, int32_t key_hi, int shift,
                                                                  uint32_t keep_slot, uint32_t* __restrict__ block_hist,
                                                                  uint32_t* __restrict__ group_rows, uint16_t* __restrict__ keys16,
                                                                  CompactCentres cc) {
    static_assert(NARROW || !COMPACT, "the 16-bit centre planes feed the 16-bit radix keys only");
    __shared__ uint32_t s_hist[4][RADIX_BINS];               // waves w, w+4, w+8, w+12 share one
    const uint32_t tid = threadIdx.x, t = blockIdx.x * HIST_THREADS + tid;
    sort_begin(p, t, gridDim.x * HIST_THREADS, keep_slot);
    if (t < SORT_SHARDS) {
        p.frame->key_min[t] = key_lo;
        p.frame->key_max[t] = key_hi;
    }
    ld.set_known_range(key_lo, key_hi);
    for (uint32_t k = tid; k < 4u * RADIX_BINS; k += HIST_THREADS) (&s_hist[0][0])[k] = 0;
    __syncthreads();
    uint32_t* hist = s_hist[(tid >> 6) & 3u];
    const uint32_t R = p.render_count;
    const RadixChunk ch = radix_chunk(R);
    // this chunk's logical elements [j0, j1) are list positions [R - j1, R - j0)
    const uint32_t j0 = min(ch.tile_begin * (uint32_t)RADIX_TILE, R), j1 = min(ch.tile_end * (uint32_t)RADIX_TILE, R);
    const uint32_t p0 = R - j1, p1 = R - j0;
    // counts one depth's radix key (hist_key counts a clamp) and returns it
    auto count = [&](int32_t k) {
        const uint32_t r = ld.hist_key(k);
        atomicAdd(&hist[(r >> shift) & 255u], 1u);
        return r;
    };
    auto scalars = [&](uint32_t begin, uint32_t end) {
        for (uint32_t i = begin + tid; i < end; i += HIST_THREADS) {
            const int32_t k = COMPACT ? compact_key_int(p, cc.k0, cc.x[i], cc.y[i], cc.z[i]) : static_key_int(p, p.cx[i], p.cy[i], p.cz[i]);
            const uint32_t r = count(k);
            if (NARROW) keys16[i] = (uint16_t)r;
            else p.keys_out[i] = k;
        }
    };
    // A unit = VPU adjacent 16-byte vectors per plane, one lane's: positions [a * UPOS, b * UPOS) as units, the ragged head and tail
    // one at a time (k_depth_key<true>'s cut).  UNITS units per thread are in flight.  COMPACT: a unit is ONE vector per plane,
    // eight positions of 16 bits.
    constexpr uint32_t VPU = (NARROW && GS_KEY_HIST_PAIR) ? 2u : 1u, UPOS = COMPACT ? 8u : 4u * VPU;
    constexpr uint32_t UNITS = VPU == 2u ? (uint32_t)(GS_KEY_HIST_PAIR ? GS_KEY_HIST_PAIR : 1) : KEY_HIST_VECS;
    const uint32_t a = (p0 + UPOS - 1u) / UPOS, b = p1 / UPOS;
    if (a < b) {
        scalars(p0, a * UPOS);
        scalars(b * UPOS, p1);
        if constexpr (COMPACT) {
            constexpr uint32_t CU = GS_KEY_HIST_C16_UNITS;
            const uint4* x8 = reinterpret_cast<const uint4*>(cc.x);
            const uint4* y8 = reinterpret_cast<const uint4*>(cc.y);
            const uint4* z8 = reinterpret_cast<const uint4*>(cc.z);
            // two positions of one word per plane -> their two radix keys as one word, the lower position in the low half
            auto two = [&](uint32_t xw, uint32_t yw, uint32_t zw) {
                const uint32_t r0 = count(compact_key_int(p, cc.k0, xw & 0xFFFFu, yw & 0xFFFFu, zw & 0xFFFFu));
                const uint32_t r1 = count(compact_key_int(p, cc.k0, xw >> 16, yw >> 16, zw >> 16));
                return r0 | (r1 << 16);
            };
            for (uint32_t u0 = a; u0 < b; u0 += CU * HIST_THREADS) {
                uint4 x[CU], y[CU], z[CU];
#pragma unroll
                for (uint32_t k = 0; k < CU; k++) {                        // (unconditional loads of clamped positions: one batch)
                    const uint32_t u = min(u0 + k * HIST_THREADS + tid, b - 1u);
                    x[k] = x8[u]; y[k] = y8[u]; z[k] = z8[u];
                }
#pragma unroll
                for (uint32_t k = 0; k < CU; k++) {
                    const uint32_t u = u0 + k * HIST_THREADS + tid;
                    if (u < b)
                        reinterpret_cast<uint4*>(keys16)[u] = make_uint4(two(x[k].x, y[k].x, z[k].x), two(x[k].y, y[k].y, z[k].y),
                                                                         two(x[k].z, y[k].z, z[k].z), two(x[k].w, y[k].w, z[k].w));
                }
            }
        } else {
            const uint4* x4 = reinterpret_cast<const uint4*>(p.cx);
            const uint4* y4 = reinterpret_cast<const uint4*>(p.cy);
            const uint4* z4 = reinterpret_cast<const uint4*>(p.cz);
            int4* o4 = reinterpret_cast<int4*>(p.keys_out);
            for (uint32_t u0 = a; u0 < b; u0 += UNITS * HIST_THREADS) {
                uint4 x[UNITS][VPU], y[UNITS][VPU], z[UNITS][VPU];
#pragma unroll
                for (uint32_t k = 0; k < UNITS; k++) {                         // (unconditional loads of clamped positions: one batch)
                    const uint32_t u = min(u0 + k * HIST_THREADS + tid, b - 1u);
#pragma unroll
                    for (uint32_t q = 0; q < VPU; q++) { x[k][q] = x4[u * VPU + q]; y[k][q] = y4[u * VPU + q]; z[k][q] = z4[u * VPU + q]; }
                }
#pragma unroll
                for (uint32_t k = 0; k < UNITS; k++) {
                    const uint32_t u = u0 + k * HIST_THREADS + tid;
                    int4 key[VPU];
#pragma unroll
                    for (uint32_t q = 0; q < VPU; q++) key[q] = static_key_int4(p, x[k][q], y[k][q], z[k][q]);
                    if (u < b) {
                        if constexpr (NARROW) {
                            uint32_t w[2u * VPU];                              // two radix keys per word, the lower position in the low half
#pragma unroll
                            for (uint32_t q = 0; q < VPU; q++) {
                                const uint32_t r0 = count(key[q].x), r1 = count(key[q].y), r2 = count(key[q].z), r3 = count(key[q].w);
                                w[2u * q] = r0 | (r1 << 16);
                                w[2u * q + 1u] = r2 | (r3 << 16);
                            }
                            if constexpr (VPU == 2u) reinterpret_cast<uint4*>(keys16)[u] = make_uint4(w[0], w[1], w[2], w[3]);
                            else reinterpret_cast<uint2*>(keys16)[u] = make_uint2(w[0], w[1]);
                        } else {
                            o4[u] = key[0];
                            count(key[0].x); count(key[0].y); count(key[0].z); count(key[0].w);
                        }
                    }
                }
            }
        }
    } else {                                               // fewer than one aligned unit
        scalars(p0, p1);
    }
    __syncthreads();
    if (tid >= RADIX_BINS || ch.tile_begin >= ch.tile_end) return;      // (a workgroup without tiles has no row)
    const uint32_t total = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
    block_hist[ch.id * RADIX_BINS + tid] = total;
    if (total) atomicAdd(&group_rows[(ch.id / RADIX_GROUP) * RADIX_BINS + tid], total);   // (k_radix_hist's two-level table)
}

__global__ void k_debug_buckets(DepthLoader ld, int32_t* out) {
    ld.prepare();
    for (uint32_t i = ld.sort_start + blockIdx.x * blockDim.x + threadIdx.x; i < ld.render_count;
         i += gridDim.x * blockDim.x)
        out[i] = (int32_t)ld.bucket(i);
}

// The int32 depth keys of a sort that stored only 16-bit radix keys (k_depth_key_hist<true>: the identity list, static integer
// mode), for the test hooks.  Nothing else: no housekeeping, no min / max - the sort's SortFrame stays as that sort left it.
__global__ __launch_bounds__(256) void k_debug_rekey(KeyParams p, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        p.keys_out[i] = static_key_int(p, p.cx[i], p.cy[i], p.cz[i]);
}

// One radix pass of a depth sort as the plan records it (sort_plan.hpp, SortPass): the buffers it may touch ...
struct PassBuffers {
    DepthLoaderArgs dl;                 // pass 0's loader
    const uint32_t* n_dev;              // the later passes' element count when it lives on the device (else nullptr: Rs)
    uint32_t Rs, val_bits;
    void* kbuf[2];                      // key / value ping-pong
    uint32_t* vbuf[2];
    uint32_t* out_tail;                 // the sorted part of the result
    uint32_t* kept_out;                 // a culling pass 0 publishes the result's length here
};
// ... pass 0 for one (CULL, IDX, NARROW) combination of the loader: packed + chunk-staged, packed, or key + value output ...
template <bool CULL, bool IDX, bool NARROW = false>
static int launch_depth_pass(const RadixExec& ex, const SortPass& ps, const PassBuffers& b, uint32_t* vo) {
    typedef DepthLoaderT<CULL, IDX, NARROW> L;
    const L d = {b.dl};
    L h = d;                            // only the histogram launch counts clamped buckets (once per element)
    h.count_clamps = 1;
    const int hs = (int)ps.hist_shift, sh = (int)ps.shift, slot = (int)ps.slot;
    const bool skip = ps.skip_hist != 0u;
    if (ps.out == SORT_OUT_PACKED && ps.chunked) return radix_pass_chunk<L, L, true>(ex, h, hs, d, ps.grid, sh, slot, vo, b.val_bits, b.kept_out, skip);
    if (ps.out == SORT_OUT_PACKED) return radix_pass_ex<L, L, uint8_t, false, false, true>(ex, h, hs, d, ps.grid, sh, slot, (uint8_t*)nullptr, vo, nullptr, 0u, b.val_bits, b.kept_out, skip);
    if constexpr (!NARROW)              // (16-bit radix keys: buckets of <= 16 bits)
        if (ps.out == SORT_OUT_KV32) return radix_pass_ex<L, L, uint32_t, true, false, false>(ex, h, hs, d, ps.grid, sh, slot, (uint32_t*)b.kbuf[0], vo, nullptr, 0u, 0u, b.kept_out, skip);
    return radix_pass_ex<L, L, uint16_t, true, false, false>(ex, h, hs, d, ps.grid, sh, slot, (uint16_t*)b.kbuf[0], vo, nullptr, 0u, 0u, b.kept_out, skip);
}
// ... and pass p, whatever it reads and writes.
static int launch_pass(const RadixExec& ex, const SortPass& ps, uint32_t p, const PassBuffers& b) {
    typedef ArrayLoader<uint32_t> A32;
    typedef ArrayLoader<uint16_t> A16;
    uint32_t* vo = ps.last ? b.out_tail : b.vbuf[p & 1];
    const void* kin = b.kbuf[(p + 1) & 1];                 // what pass p - 1 wrote
    const uint32_t* vin = b.vbuf[(p + 1) & 1];
    const int hs = (int)ps.hist_shift, sh = (int)ps.shift, slot = (int)ps.slot;
    const bool packs = ps.out == SORT_OUT_PACKED;
    switch (ps.in) {
    case SORT_IN_DEPTH:
        if (ps.in_narrow) return launch_depth_pass<false, false, true>(ex, ps, b, vo);   // (a known-range sort: the identity list, no cull)
        if (ps.in_cull) return ps.in_idx ? launch_depth_pass<true, true>(ex, ps, b, vo) : launch_depth_pass<true, false>(ex, ps, b, vo);
        return ps.in_idx ? launch_depth_pass<false, true>(ex, ps, b, vo) : launch_depth_pass<false, false>(ex, ps, b, vo);
    case SORT_IN_PACKED: {
        const PackedLoader pk = {vin, b.n_dev, b.Rs, b.val_bits};
        const A32 ph = {vin, nullptr, b.n_dev, b.Rs};      // (the histogram reads the packed words as plain keys)
        if (ps.chunked && packs) return radix_pass_chunk<A32, PackedLoader, true>(ex, ph, hs, pk, ps.grid, sh, slot, vo, b.val_bits);
        if (ps.chunked) return radix_pass_chunk<A32, PackedLoader, false>(ex, ph, hs, pk, ps.grid, sh, slot, vo, 0u);
        if (packs) return radix_pass_ex<A32, PackedLoader, uint8_t, false, false, true>(ex, ph, hs, pk, ps.grid, sh, slot, (uint8_t*)nullptr, vo, nullptr, 0u, b.val_bits);
        return radix_pass_ex<A32, PackedLoader, uint8_t, false, false, false>(ex, ph, hs, pk, ps.grid, sh, slot, (uint8_t*)nullptr, vo, nullptr, 0u, 0u);
    }
    case SORT_IN_KEYS32: {
        const A32 al = {(const uint32_t*)kin, vin, b.n_dev, b.Rs};
        if (ps.out == SORT_OUT_FINAL) return radix_pass_ex<A32, A32, uint32_t, false, false, false>(ex, al, hs, al, ps.grid, sh, slot, (uint32_t*)nullptr, vo, nullptr, 0u, 0u);
        if (packs) return radix_pass_ex<A32, A32, uint8_t, false, false, true>(ex, al, hs, al, ps.grid, sh, slot, (uint8_t*)nullptr, vo, nullptr, 0u, b.val_bits);
        return radix_pass_ex<A32, A32, uint32_t, true, false, false>(ex, al, hs, al, ps.grid, sh, slot, (uint32_t*)b.kbuf[p & 1], vo, nullptr, 0u, 0u);
    }
    case SORT_IN_KEYS16: {
        const A16 al = {(const uint16_t*)kin, vin, b.n_dev, b.Rs};
        if (ps.out == SORT_OUT_FINAL) return radix_pass_ex<A16, A16, uint16_t, false, false, false>(ex, al, hs, al, ps.grid, sh, slot, (uint16_t*)nullptr, vo, nullptr, 0u, 0u);
        return radix_pass_ex<A16, A16, uint16_t, true, false, false>(ex, al, hs, al, ps.grid, sh, slot, (uint16_t*)b.kbuf[p & 1], vo, nullptr, 0u, 0u);
    }
    }
    GS_REQUIRE(false, "sort plan: unknown loader");
}

static inline uint32_t grid_for(uint32_t n, uint32_t per_block, uint32_t cap) {
    uint32_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return g > cap ? cap : g;
}

#ifdef GS_RADIX_PROFILE
extern "C" int gs_debug_radix_prof(void* dst) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_radix_prof), sizeof(g_radix_prof), 0, hipMemcpyDeviceToHost);
}
#endif

// Every buffer of a sorter whose size depends on its capacity (gs_internal.hpp, CapBuf): gs_sorter_create allocates from this
// list, gs_sorter_resize moves the sorter from the list of one capacity to the list of another.  Needs the sorter's flags.
std::vector<CapBuf> gs_sorter_capacity_list(gs_sorter* s, uint32_t capacity) {
    const size_t n = capacity, b4 = n * 4;
    std::vector<CapBuf> l;
    auto A = [&](DevBuf& b, size_t bytes, uint32_t elem, CapRole role) { l.push_back(CapBuf{&b, bytes, elem, role}); };
    A(s->cx, b4 + 16, 4, CAP_PLANE); A(s->cy, b4 + 16, 4, CAP_PLANE); A(s->cz, b4 + 16, 4, CAP_PLANE);   // (+16: k_cull_front reads whole 16-byte vectors)
    A(s->caos, n * 16, 16, CAP_PLANE);
    if (s->flags & GS_SORT_DYNAMIC) { A(s->cw, b4 + 16, 4, CAP_PLANE); A(s->scene_idx, b4 + 16, 4, CAP_PLANE); }   // (+16: as above)
    A(s->keys, b4, 4, CAP_SCRATCH); A(s->keyA, b4, 4, CAP_SCRATCH); A(s->keyB, b4, 4, CAP_SCRATCH);
    A(s->valA, b4, 4, CAP_SCRATCH); A(s->valB, b4, 4, CAP_SCRATCH); A(s->sorted, b4, 4, CAP_SCRATCH);
    A(s->keys16, n * 2 + 16, 2, CAP_SCRATCH);
    // by their first users: a sort from a list, from distances, under a cull, of a gathered list; the debug reads; the 16-bit
    // centre planes (sorter_update_compact builds them from the int32 planes)
    // (they size themselves from max_count where they allocate; the list only says that they go with the capacity)
    for (DevBuf* b : {&s->idx_in, &s->precomputed, &s->pay_in, &s->debug, &s->keep_mask, &s->mask_copy, &s->cx16, &s->cy16, &s->cz16})
        A(*b, 0, 0, CAP_LAZY);
    return l;
}

extern "C" {

int gs_sorter_create(gs_context* ctx, uint32_t max_splat_count, uint32_t flags, uint32_t precision_bits,
                     gs_sorter** out) {
    GS_REQUIRE(ctx && out, "ctx / out == NULL");
    *out = nullptr;
    GS_REQUIRE(max_splat_count > 0, "max_splat_count == 0");
    GS_REQUIRE((flags & ~(GS_SORT_INTEGER | GS_SORT_DYNAMIC)) == 0, "unknown sorter flags");
    const uint32_t max_bits = (flags & GS_SORT_INTEGER) ? 20u : 24u;   // src/Viewer.js:208-210
    GS_REQUIRE(precision_bits >= 10 && precision_bits <= max_bits, "precision outside the Viewer's clamp (10..20 int, 10..24 float)");
    ScopedDevice sd(ctx->device);
    gs_sorter* s = new (std::nothrow) gs_sorter();
    if (!s) return GS_ERR_NOMEM;
    s->ctx = ctx;
    s->handover.owner = s;
    s->max_count = max_splat_count;
    s->flags = flags;
    s->precision = precision_bits;
    int st = GS_OK;
    auto A = [&](DevBuf& b, size_t bytes) { if (st == GS_OK) st = b.alloc(bytes); };
    for (const CapBuf& c : gs_sorter_capacity_list(s, max_splat_count))   // everything the capacity sizes
        if (c.role != CAP_LAZY) A(*c.buf, c.bytes);
    if (flags & GS_SORT_DYNAMIC) A(s->scene_rows, sizeof(SceneRows));
    A(s->frame, 2 * sizeof(SortFrame));
    if (st == GS_OK) st = s->radix.init();
    if (st == GS_OK && (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess ||
                        hipEventCreateWithFlags(&s->ev_consumed, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&s->ev_handover, hipEventDisableTiming) != hipSuccess)) {
        gs_set_error("hipEventCreate failed");
        st = GS_ERR_HIP;
    }
    if (st == GS_OK) {
        SortFrame init[2];
        for (SortFrame& f : init) {
            for (uint32_t k = 0; k < SORT_SHARDS; k++) { f.key_min[k] = KEY_MIN_INIT; f.key_max[k] = KEY_MAX_INIT; }
            f.clamped = f.kept = 0;
        }
        if (hipMemcpy(s->frame.p, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(s->radix.digit_total.p, 0, sizeof(uint32_t) * RADIX_TOTAL_WORDS) != hipSuccess) {
            gs_set_error("initialising the sorter scratch failed");
            st = GS_ERR_HIP;
        }
    }
    if (st == GS_OK) {
        if (ctx->serial) {
            s->stream = ctx->stream;
        } else if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess) {
            s->own_stream = true;
        } else {
            gs_set_error("hipStreamCreate(sorter) failed");
            st = GS_ERR_HIP;
        }
    }
    if (st != GS_OK) {
        gs_sorter_destroy(s);
        return st;
    }
    ctx->live_sorters.push_back(s);
    *out = s;
    return GS_OK;
}

void gs_sorter_destroy(gs_sorter* s) {
    if (!s) return;
    std::vector<gs_sorter*>& live = s->ctx->live_sorters;
    live.erase(std::remove(live.begin(), live.end(), s), live.end());
    handover_dropped(s->handover);
    ScopedDevice sd(s->ctx->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    (void)hipStreamSynchronize(s->ctx->stream);        // a draw may still be reading `sorted`
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->ev_consumed) (void)hipEventDestroy(s->ev_consumed);
    if (s->ev_handover) (void)hipEventDestroy(s->ev_handover);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

static void sorter_tell_mesh(gs_sorter* s);   // (defined with gs_sorter_bind_mesh)

// The switches of this file (sort_plan.hpp, SortSwitches), read here and nowhere else: once per process, at the first upload or sort.
static SortSwitches sort_switches() {
    static const SortSwitches sw = [] {
        SortSwitches w = {};
        const char* vis_front = getenv("GSPLAT_VIS_FRONT");
        w.tree_no_fuse = getenv("GSPLAT_TREE_NO_FUSE") != nullptr;
        w.vis_front = !vis_front ? 0u : vis_front[0] == 's' ? 1u : 2u;
        w.no_pack = getenv("GSPLAT_NO_SORT_PACK") != nullptr;
        w.no_chunk = getenv("GSPLAT_NO_SORT_CHUNK") != nullptr;
        w.no_known_range = getenv("GSPLAT_NO_KNOWN_RANGE") != nullptr;
        w.no_narrow_keys = getenv("GSPLAT_NO_NARROW_KEYS") != nullptr;
        w.no_compact_centres = getenv("GSPLAT_NO_COMPACT_CENTRES") != nullptr;
        return w;
    }();
    return sw;
}

// The extreme set follows the centres (static integer sorters): called after centers_version moved on, with the stream idle.
// Rows [from, end) of `caos` were written (zero_fill: with zeros), old_uploaded rows were in use before.  hull(old U new) =
// hull(set(old) U new): a range behind the old rows extends the set, a range that overwrites old rows rebuilds it from every row.
// The rows are read back from the device - one path for centres from the host, from an asset's decode and for never-written gaps.
static int sorter_update_extreme(gs_sorter* s, uint32_t from, uint32_t end, uint32_t old_uploaded, bool zero_fill) {
    if (s->flags != GS_SORT_INTEGER || sort_switches().no_known_range) return GS_OK;
    const bool current = s->extreme_ok && s->extreme_version + 1u == s->centers_version;   // it covered the centres until now
    const bool append = from >= old_uploaded;
    if (append && !current) {                              // no set to extend: none until an overwrite rebuilds it
        s->extreme_ok = false;
        return GS_OK;
    }
    const uint32_t first = append ? old_uploaded : 0u, last = end > old_uploaded ? end : old_uploaded;
    std::vector<int32_t> rows, out;
    try {
        if (zero_fill && append) rows.assign(4, 0);        // (0, 0, 0), as often as it likes
        else rows.resize((size_t)(last - first) * 4);
    } catch (const std::bad_alloc&) {
        s->extreme_ok = false;
        return GS_OK;
    }
    if (!(zero_fill && append) && last > first) {
        GS_HIP(hipMemcpyAsync(rows.data(), s->caos.as<uint4>() + first, (size_t)(last - first) * 16, hipMemcpyDeviceToHost, s->stream));
        GS_HIP(hipStreamSynchronize(s->stream));
    }
    const bool prior = append && !s->extreme.empty();
    s->extreme_ok = gs_extreme_set(prior ? s->extreme.data() : nullptr, prior ? s->extreme.size() / 4 : 0, rows.data(), rows.size() / 4,
                                   GS_EXTREME_CAP, out);
    s->extreme.swap(out);
    s->extreme_version = s->centers_version;
    return GS_OK;
}

// The 16-bit centre planes follow the centres and their extreme set: called after sorter_update_extreme, with the stream idle and
// the int32 planes of [from, end) written.  Valid only with a valid extreme set whose per-axis extent fits 16 bits
// (gs_compact_offsets).  The same offsets as for the version before: only [from, end) is rebuilt - with the never-written gap in
// front of a range that starts behind the old_uploaded rows in use before, which the set counts too; else every uploaded position.
// The builder counts what does not fit - a hull vertex missing from the set then costs the planes, never a key.
static int sorter_update_compact(gs_sorter* s, uint32_t from, uint32_t end, uint32_t old_uploaded) {
    const bool was_current = s->c16_ok && s->c16_version + 1u == s->centers_version;
    s->c16_ok = false;
    if (s->flags != GS_SORT_INTEGER || sort_switches().no_compact_centres || s->uploaded == 0u) return GS_OK;
    if (!s->extreme_ok || s->extreme_version != s->centers_version) return GS_OK;
    int32_t off[3];
    if (!gs_compact_offsets(s->extreme.data(), s->extreme.size() / 4, off)) return GS_OK;
    const size_t bytes = (size_t)s->max_count * 2 + 16;
    bool fresh[3];
    GS_TRY(s->cx16.ensure(bytes, &fresh[0])); GS_TRY(s->cy16.ensure(bytes, &fresh[1])); GS_TRY(s->cz16.ensure(bytes, &fresh[2]));
    GS_TRY(s->c16_bad.ensure(4));
    const bool keep = was_current && !fresh[0] && !fresh[1] && !fresh[2] && off[0] == s->c16_off[0] && off[1] == s->c16_off[1] &&
                      off[2] == s->c16_off[2];
    from = keep ? std::min(from, old_uploaded) : 0u;
    if (!keep) end = s->uploaded;
    hipStream_t st = s->stream;
    uint32_t bad = 1u;
    GS_HIP(hipMemsetAsync(s->c16_bad.p, 0, 4, st));
    hipLaunchKernelGGL(k_compact_centres, dim3(grid_for(end - from, 1024, 4096)), dim3(256), 0, st, s->cx.as<int32_t>(), s->cy.as<int32_t>(),
                       s->cz.as<int32_t>(), from, end, off[0], off[1], off[2], s->cx16.as<uint16_t>(), s->cy16.as<uint16_t>(),
                       s->cz16.as<uint16_t>(), s->c16_bad.as<uint32_t>());
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(&bad, s->c16_bad.p, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    memcpy(s->c16_off, off, sizeof(off));
    s->c16_version = s->centers_version;
    s->c16_ok = bad == 0u;
    return GS_OK;
}

// A sort that stored 16-bit radix keys left `keys` stale, and gs_sorter_debug_read (selectors 0 and 1) describes the sort that ran:
// its depth keys are rebuilt here, on the sorter's stream, from the planes and the coefficients of that sort - before a selector
// reads them, and before an upload overwrites the planes they come from (set-up calls: one streaming kernel is free there).
static int sorter_refresh_keys(gs_sorter* s) {
    if (!s->keys_stale) return GS_OK;
    KeyParams kp = {};
    kp.cx = s->cx.as<uint32_t>(); kp.cy = s->cy.as<uint32_t>(); kp.cz = s->cz.as<uint32_t>();
    kp.keys_out = s->keys.as<int32_t>();
    kp.mode = MODE_INT;
    kp.im0 = s->stale_im[0]; kp.im1 = s->stale_im[1]; kp.im2 = s->stale_im[2];
    hipLaunchKernelGGL(k_debug_rekey, dim3(grid_for(s->stale_count, 1024, 2048)), dim3(256), 0, s->stream, kp, s->stale_count);
    GS_HIP(hipGetLastError());
    s->keys_stale = false;
    return GS_OK;
}

int gs_sorter_upload_centers(gs_sorter* s, uint32_t from, uint32_t count, const void* centers_aos4,
                             const uint32_t* scene_indexes) {
    GS_REQUIRE(s && centers_aos4, "sorter / centers == NULL");
    GS_REQUIRE((uint64_t)from + count <= s->max_count, "range exceeds max_splat_count");
    GS_REQUIRE(!(s->flags & GS_SORT_DYNAMIC) || scene_indexes, "dynamic sorter needs scene_indexes");
    if (count == 0) return GS_OK;
    ScopedDevice sd(s->ctx->device);
    GS_TRY(sorter_refresh_keys(s));                        // (ordered before the copies below)
    GS_HIP(hipMemcpyAsync(s->caos.as<uint4>() + from, centers_aos4, (size_t)count * 16, hipMemcpyHostToDevice, s->stream));
    return gs_sorter_commit_centers(s, from, count, scene_indexes);
}

}  // extern "C"

// The AoS x4 centres of [from, from + count) are in `caos` (enqueued on the sorter's stream by a copy from the host or by
// asset_decode.hip's k_asset_centers): the SoA planes, the scene indexes and the bookkeeping of a `centers` message.
int gs_sorter_commit_centers(gs_sorter* s, uint32_t from, uint32_t count, const uint32_t* scene_indexes) {
    hipStream_t st = s->stream;
    GS_TRY(sorter_refresh_keys(s));                        // (an asset's decode comes straight here: before the planes change)
    uint4* aos = s->caos.as<uint4>() + from;               // kept: index-list sorts gather 16 bytes per splat from it
    hipLaunchKernelGGL(k_aos4_to_soa, dim3(grid_for(count, 256, 4096)), dim3(256), 0, st, aos, count,
                       from, s->cx.as<uint32_t>(), s->cy.as<uint32_t>(), s->cz.as<uint32_t>(),
                       (s->flags & GS_SORT_DYNAMIC) ? s->cw.as<uint32_t>() : nullptr);
    GS_HIP(hipGetLastError());
    if (s->flags & GS_SORT_DYNAMIC)
        GS_HIP(hipMemcpyAsync(s->scene_idx.as<uint32_t>() + from, scene_indexes, (size_t)count * 4, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));   // staging and the caller's buffers are reusable on return
    const uint32_t old_uploaded = s->uploaded;
    if (from + count > s->uploaded) s->uploaded = from + count;   // uploadedSplatCount, SortWorker.js:97
    s->centers_version++;
    GS_TRY(sorter_update_extreme(s, from, from + count, old_uploaded, false));
    GS_TRY(sorter_update_compact(s, from, from + count, old_uploaded));
    sorter_tell_mesh(s);                                   // (more centres than the bound mesh holds: no position map, no derived mask)
    return GS_OK;
}

// Every state of a sorter that names splats by their numbering: the resident result, a gathered (or planned) list, the per-tree
// payload caches, the mask a visibility-culled sort consumed, the stale-key state and device distances.
static void sorter_forget_numbering(gs_sorter* s) {
    handover_dropped(s->handover);
    s->has_result = false;
    s->result_mesh = nullptr; s->result_unmap = nullptr; s->result_frame = nullptr; s->result_payload_max = 0;
    s->last_render = s->last_sort = s->last_passes = 0;
    s->last_in = SortPlanIn(); s->last_plan = SortPlan();
    s->leaf_cache_tree = 0; s->leaf_cache_mesh = nullptr;
    s->keys_stale = false; s->stale_count = 0;
    s->dev_distances = false; s->dev_distances_count = 0;
    s->mask_copy.release();
}

void gs_sorter_mesh_edited(gs_sorter* s) {
    sorter_forget_numbering(s);
    sorter_tell_mesh(s);
}

// The bound mesh changed its storage order and kept the caller's numbering (gs_mesh_reorder): what goes is what the sorter keeps in
// storage order - the resident result (its payloads are storage positions), the leaf-ordered payload cache and the mask of the
// last visibility-culled sort.  Gathered lists, trees, stale keys and device distances are in the caller's numbering and stay.
void gs_sorter_mesh_reordered(gs_sorter* s) {
    s->has_result = false;
    s->result_mesh = nullptr; s->result_unmap = nullptr; s->result_frame = nullptr; s->result_payload_max = 0;
    s->last_render = s->last_sort = s->last_passes = 0;
    s->leaf_cache_tree = 0; s->leaf_cache_mesh = nullptr;
    s->mask_copy.release();
    sorter_tell_mesh(s);
}

extern "C" {

int gs_sorter_remove(gs_sorter* s, const uint32_t* ranges, uint32_t n_ranges, const uint32_t* scene_remap, uint32_t scene_remap_count) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    if (n_ranges == 0) return GS_OK;
    GS_REQUIRE(ranges != nullptr, "ranges == NULL");
    GS_REQUIRE(n_ranges <= GS_MAX_SCENES, "gs_sorter_remove: more than GS_MAX_SCENES ranges");
    GS_REQUIRE(scene_remap || scene_remap_count == 0, "gs_sorter_remove: scene_remap == NULL with a count");
    GS_REQUIRE(scene_remap_count <= GS_MAX_SCENES, "gs_sorter_remove: scene_remap_count > GS_MAX_SCENES");
    for (uint32_t k = 0; k < scene_remap_count; k++) GS_REQUIRE(scene_remap[k] < GS_MAX_SCENES, "gs_sorter_remove: scene_remap entry >= GS_MAX_SCENES");
    const RemovePlan plan = plan_remove(std::vector<SlotRange>(), SlottedRanges(), s->uploaded, s->max_count, false, ranges, n_ranges);
    if (plan.refused) {
        gs_set_error("invalid argument: gs_sorter_remove: %s", plan.refused);
        return GS_ERR_INVALID;
    }
    if (plan.removed == 0) return GS_OK;                    // every range lies beyond the uploaded centres
    ScopedDevice sd(s->ctx->device);
    hipStream_t st = s->stream;
    GS_HIP(hipStreamSynchronize(st));                      // the sort in flight
    if (s->ctx->stream != st) GS_HIP(hipStreamSynchronize(s->ctx->stream));   // a draw may still be reading `sorted`
    // the rows as uploaded move down (and the scene indexes, through the table); the SoA planes, the extreme set and the 16-bit
    // planes are derived from the surviving rows as an upload derives them
    const uint32_t old_end = s->uploaded, new_end = plan.uploaded, base = plan.cuts[0].begin & ~3u;
    GS_TRY(s->staging.ensure((size_t)(new_end - base) * 16 + 16));
    const RemoveMap map = gs_remove_map(plan, scene_remap, scene_remap_count);
    GS_TRY(gs_remove_compact(st, map, s->caos.p, 16, GS_REMOVE_PLAIN, base, new_end, old_end, s->staging.p));
    if (s->flags & GS_SORT_DYNAMIC) GS_TRY(gs_remove_compact(st, map, s->scene_idx.p, 4, GS_REMOVE_SCENES, base, new_end, old_end, s->staging.p));
    if (new_end > base) {
        hipLaunchKernelGGL(k_aos4_to_soa, dim3(grid_for(new_end - base, 256, 4096)), dim3(256), 0, st, s->caos.as<uint4>() + base, new_end - base,
                           base, s->cx.as<uint32_t>(), s->cy.as<uint32_t>(), s->cz.as<uint32_t>(),
                           (s->flags & GS_SORT_DYNAMIC) ? s->cw.as<uint32_t>() : nullptr);
        GS_HIP(hipGetLastError());
    }
    GS_HIP(hipStreamSynchronize(st));
    s->uploaded = new_end;
    s->centers_version++;
    sorter_forget_numbering(s);
    s->extreme.clear();                                    // no centres: the empty set ...
    s->extreme_ok = true;
    s->extreme_version = s->centers_version;
    if (new_end) GS_TRY(sorter_update_extreme(s, 0, new_end, new_end, false));   // ... else rebuilt from every surviving row
    GS_TRY(sorter_update_compact(s, 0, new_end, new_end));
    sorter_tell_mesh(s);
    return GS_OK;
}

// The sorter's half of gs_mesh_resize (mesh_edit.hip: gs_capacity_move).  The rows as uploaded, the SoA planes and
// the scene indexes are copied; the extreme set depends on the rows alone and stays; the 16-bit planes are built again from the
// int32 planes, as an upload builds them for new buffers.
int gs_sorter_resize(gs_sorter* s, uint32_t max_splat_count) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    if (max_splat_count == s->max_count && !s->scratch_lost) return GS_OK;
    GS_REQUIRE(max_splat_count > 0, "gs_sorter_resize: max_splat_count == 0");
    if (max_splat_count < s->uploaded) {
        gs_set_error("invalid argument: gs_sorter_resize: max_splat_count %u is below the uploaded splat count %u (remove centres first)",
                     max_splat_count, s->uploaded);
        return GS_ERR_INVALID;
    }
    ScopedDevice sd(s->ctx->device);
    hipStream_t st = s->stream;
    GS_HIP(hipStreamSynchronize(st));                      // the sort in flight
    if (s->ctx->stream != st) GS_HIP(hipStreamSynchronize(s->ctx->stream));   // a draw may still be reading `sorted`
    sorter_forget_numbering(s);                            // whatever comes of it, the result and the lists go with their buffers
    s->consumer_pending = false;                           // (the context's stream is idle: no draw reads `sorted`)
    int status = gs_capacity_move(st, gs_sorter_capacity_list(s, s->max_count), gs_sorter_capacity_list(s, max_splat_count), s->uploaded);
    s->scratch_lost = status == GS_CAPACITY_SCRATCH_LOST;  // (not even the old scratch came back: sorts are refused)
    if (s->scratch_lost) status = GS_ERR_NOMEM;
    if (status == GS_OK) s->max_count = max_splat_count;
    s->c16_ok = false;                                     // the 16-bit planes went with the scratch: every uploaded position again
    const int compact = sorter_update_compact(s, 0, s->uploaded, s->uploaded);
    if (compact != GS_OK && compact != GS_ERR_NOMEM) return compact;   // (no room for the 16-bit planes: sorts read the int32 ones)
    sorter_tell_mesh(s);
    return status;
}

int gs_sorter_set_uploaded_count(gs_sorter* s, uint32_t count) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    GS_REQUIRE(count <= s->max_count, "count exceeds max_splat_count");
    if (count <= s->uploaded) return GS_OK;
    ScopedDevice sd(s->ctx->device);
    hipStream_t st = s->stream;
    const size_t from = s->uploaded, n = count - s->uploaded;
    GS_HIP(hipMemsetAsync(s->caos.as<uint4>() + from, 0, n * 16, st));
    DevBuf* planes[] = {&s->cx, &s->cy, &s->cz, &s->cw, &s->scene_idx};
    for (DevBuf* b : planes)
        if (b->p) GS_HIP(hipMemsetAsync(b->as<uint32_t>() + from, 0, n * 4, st));
    GS_HIP(hipStreamSynchronize(st));
    s->uploaded = count;
    s->centers_version++;
    GS_TRY(sorter_update_extreme(s, (uint32_t)from, count, (uint32_t)from, true));
    GS_TRY(sorter_update_compact(s, (uint32_t)from, count, (uint32_t)from));
    sorter_tell_mesh(s);
    return GS_OK;
}

static int sorter_collect_stats(gs_sorter* s, gs_sort_stats* stats) {
    SortFrame f;
    GS_HIP(hipMemcpyAsync(&f, s->frame.as<SortFrame>() + s->frame_index, sizeof(f), hipMemcpyDeviceToHost, s->stream));
    GS_HIP(hipStreamSynchronize(s->stream));
    float ms = 0.f;
    if (s->timed_sort) GS_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    int32_t key_lo = f.lo(), key_hi = f.hi();
    if (s->last_sort == 0) {                       // nothing was keyed: the frame belongs to an earlier sort
        key_lo = KEY_MIN_INIT;
        key_hi = KEY_MAX_INIT;
        f.clamped = 0;
    }
    stats->device_ms = ms;
    stats->key_min = key_lo;
    stats->key_max = key_hi;
    stats->clamped = f.clamped;
    stats->passes = s->last_passes;
    stats->result_count = s->last_plan.count_on_device ? f.kept : s->last_render;
    return f.clamped ? GS_WARN_KEY_CLAMPED : GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// One sort, in steps: sort_check (the inputs of the plan, the refusals) -> plan_sort (sort_plan.cpp: everything that is decided) ->
// sort_stage_inputs -> launch_front_end -> run_radix_passes -> sort_finish, which all act on the plan and change none of it.
// ---------------------------------------------------------------------------------------------------
static bool sorter_mesh_alive(const gs_context* ctx, const gs_mesh* m) {   // a sorter never dereferences a destroyed mesh
    for (const gs_mesh* l : ctx->live_meshes)
        if (l == m) return m != nullptr;
    return false;
}

// The call as it came in, and what of it sort_check worked out for the launch code
struct SortCall {
    const float* mvp;
    const uint32_t* indexes_to_sort;
    bool device_list;                  // the list is what gs_tree_gather left (or planned) in idx_in
    const void* precomputed;
    const float* transforms;
    const uint32_t* list_count_dev;    // the list's real length lives on the device (asynchronous gs_tree_gather); R bounds it
    uint32_t sort_count, render_count;
    int32_t im[3];                     // the static integer key's coefficients: (int)(mvp[k]*1000.0), k = 2,6,10  (sorter.cpp:64)
    const uint32_t *map, *unmap;       // a bound mesh stores its splats in its own (Morton) order: hand it positions in that order
};

// 1. the inputs of the plan, from the sorter, the call and the bound mesh - and the refusals, in the order and at the places they
// have always had between the calls with side effects
static int sort_check(gs_sorter* s, SortCall& c, SortPlanIn& in) {
    in = SortPlanIn();
    in.flags = s->flags; in.precision = s->precision; in.uploaded = s->uploaded;
    in.frustum_cull = s->frustum_cull; in.visibility_cull = s->visibility_cull;
    in.clean_slot = s->clean_slot;
    in.pending_gather = s->handover.state == HANDOVER_PLANNED; in.pending_keep_zeroed = s->handover.keep_zeroed;
    in.extreme_current = s->extreme_ok && s->extreme_version == s->centers_version && !s->extreme.empty();
    in.c16_current = s->c16_ok && s->c16_version == s->centers_version;
    in.sort_count = c.sort_count; in.render_count = c.render_count;
    in.list = c.device_list ? SORT_LIST_DEVICE : c.indexes_to_sort ? SORT_LIST_HOST : SORT_LIST_IDENTITY;
    in.precomputed = !c.precomputed ? SORT_PRE_NONE : c.precomputed == GS_PRECOMPUTED_DEVICE ? SORT_PRE_DEVICE : SORT_PRE_HOST;
    in.count_on_device = c.list_count_dev != nullptr;
    in.cu_count = (uint32_t)s->ctx->cu_count;
    in.sw = sort_switches();
    if (in.precomputed == SORT_PRE_DEVICE) {
        GS_REQUIRE(s->dev_distances, "GS_PRECOMPUTED_DEVICE: no gs_mesh_compute_distances has handed distances to this sorter");
        GS_REQUIRE(s->dev_distances_count >= s->uploaded, "GS_PRECOMPUTED_DEVICE: fewer distances than the sorter's uploaded splats");
        GS_REQUIRE(s->dev_distances_integer == ((s->flags & GS_SORT_INTEGER) != 0),
                   "GS_PRECOMPUTED_DEVICE: the distances were computed for the other GS_SORT_INTEGER setting");
    }
    const SortCounts n = sort_counts(in);
    const bool dynamic = (s->flags & GS_SORT_DYNAMIC) != 0;
    GS_REQUIRE(n.Rs <= n.R, "splatSortCount > splatRenderCount");
    GS_REQUIRE(!dynamic || c.transforms, "dynamic sorter needs transforms");
    GS_REQUIRE(!c.list_count_dev || (c.device_list && n.Rs == n.R && !dynamic && !c.precomputed),
               "a gathered list whose length lives on the device needs a full sort of a static scene without precomputed distances");
    GS_REQUIRE(!(n.cull || n.vis_cull) || (n.Rs == n.R && !c.precomputed),
               "a per-splat cull needs a full sort (splatSortCount == splatRenderCount) without precomputed distances");
    GS_REQUIRE(!n.cull || !dynamic, "the per-splat frustum cull needs a static scene (a dynamic-mode sorter culls by visibility only)");
    if (!sorter_mesh_alive(s->ctx, s->bound_mesh)) s->bound_mesh = nullptr;   // the mesh may have been destroyed since the bind
    const gs_mesh* mesh = s->bound_mesh;
    c.map = mesh ? gs_mesh_payload_map(s->bound_mesh, s->uploaded) : nullptr;
    if (n.vis_cull) {
        GS_REQUIRE(mesh && mesh->projection_pending && mesh->uploaded >= s->uploaded,
                   "the visibility cull needs gs_sorter_bind_mesh and a gs_mesh_project of this frame's camera before the sort");
        GS_REQUIRE(!c.indexes_to_sort && !c.device_list, "the visibility cull sorts the identity list (pass indexes_to_sort = NULL)");
        // (projected_cam is the camera of the gs_mesh_project this sort consumes)
        const gs_camera& pc = mesh->projected_cam;
        const uint32_t rows_total = (pc.height + GS_TILE - 1u) / GS_TILE;
        in.mesh_strip = !(pc.tile_row_begin == 0u && (pc.tile_row_end == 0u || pc.tile_row_end >= rows_total));
        in.mesh_lazy_mask = mesh->set().vis_orig_lazy;
    }
    c.unmap = c.map ? gs_mesh_payload_unmap(s->bound_mesh) : nullptr;
    in.mesh_map = c.map != nullptr;
    in.mesh_uploaded = mesh ? mesh->uploaded : 0u;
    for (int k = 0; k < 3; k++) c.im[k] = trunc_f64_i32((double)c.mvp[2 + 4 * k] * 1000.0);
    if (sort_wants_key_range(in)) in.range_ok = gs_key_range(s->extreme.data(), s->extreme.size() / 4, c.im, &in.range_lo, &in.range_hi);
    return GS_OK;
}

// The per-scene key rows of a dynamic sort: computeMatMul4x4ThirdRow (sorter.cpp:11-15), fp32, left-to-right, no contraction;
// then x1000 in double
static int store_scene_rows(gs_sorter* s, const float* mvp, const float* transforms) {
    SceneRows rows;
    for (uint32_t sc = 0; sc < GS_MAX_SCENES; sc++) {
        const float* b = transforms + 16 * sc;
        for (int c = 0; c < 4; c++) {
            volatile float acc = mvp[2] * b[4 * c + 0];
            acc = acc + mvp[6] * b[4 * c + 1];
            acc = acc + mvp[10] * b[4 * c + 2];
            acc = acc + mvp[14] * b[4 * c + 3];
            rows.fm[sc][c] = acc;
            rows.im[sc][c] = trunc_f64_i32((double)rows.fm[sc][c] * 1000.0);
        }
    }
    k_store_scene_rows<<<1, 256, 0, s->stream>>>(rows, s->scene_rows.as<SceneRows>());
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// 2. stream ordering and input staging: what the sort waits for, the index list, the distances, the scene rows, KeyParams
static int sort_stage_inputs(gs_sorter* s, const SortCall& c, const SortPlan& pl, KeyParams& kp) {
    gs_context* ctx = s->ctx;
    hipStream_t st = s->stream;
    const float* mvp = c.mvp;
    const bool dynamic = (s->flags & GS_SORT_DYNAMIC) != 0;
    if (pl.vis_cull && s->bound_mesh->ev_p1 && ctx->aux != st) GS_HIP(hipStreamWaitEvent(st, s->bound_mesh->ev_p1, 0));   // the mask it reads
    if (ctx->fork_join && st != ctx->stream) {
        // serial frames on a multi-stream context: this sort starts when everything the context's stream holds now (the previous
        // frame's draw) has finished, then runs beside this frame's vertex stage
        GS_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
        GS_HIP(hipStreamWaitEvent(st, ctx->ev_fork, 0));
    }
    if (s->consumer_pending) {           // a draw enqueued on ctx->stream still reads the previous result
        GS_HIP(hipStreamWaitEvent(st, s->ev_consumed, 0));
        s->consumer_pending = false;
    }

    if (c.device_list) {
        kp.idx_in = s->idx_in.as<uint32_t>();              // written by gs_tree_gather on this stream ...
        if (pl.gather == SORT_GATHER_PLAIN) {              // ... or only planned by it (tree.hip): the copy is ours, here or fused
            GS_TRY(gs_tree_copy_plain(s->handover.tree->owner, s->idx_in.as<uint32_t>(), st));
            handover_copied(s->handover);
        }
    } else {
        // a sort that does not consume the gathered list may destroy what a gather left for a later gs_sorter_sort_gathered
        if (pl.cull) handover_keep_mask_rewritten(s->handover);
        if (c.indexes_to_sort) {
            handover_list_overwritten(s->handover);
            GS_TRY(s->idx_in.ensure((size_t)s->max_count * 4));
            if (pl.R) GS_HIP(hipMemcpyAsync(s->idx_in.p, c.indexes_to_sort, (size_t)pl.R * 4, hipMemcpyHostToDevice, st));
            kp.idx_in = s->idx_in.as<uint32_t>();
        }
    }
    kp.mode = ((s->flags & GS_SORT_INTEGER) ? MODE_INT : 0) | (dynamic ? MODE_DYNAMIC : 0) | (c.precomputed ? MODE_PRECOMPUTED : 0);
    if (c.precomputed) {
        GS_TRY(s->precomputed.ensure((size_t)s->max_count * 4));
        if (c.precomputed != GS_PRECOMPUTED_DEVICE) {   // (the device hand-over: gs_mesh_compute_distances wrote the buffer in place)
            GS_HIP(hipMemcpyAsync(s->precomputed.p, c.precomputed, (size_t)s->uploaded * 4, hipMemcpyHostToDevice, st));
            s->dev_distances = false;
        }
        kp.precomputed = s->precomputed.as<uint32_t>();
    }
    if (dynamic && !c.precomputed) {
        GS_TRY(store_scene_rows(s, mvp, c.transforms));
        kp.rows = s->scene_rows.as<SceneRows>();
    }
    kp.cx = s->cx.as<uint32_t>(); kp.cy = s->cy.as<uint32_t>(); kp.cz = s->cz.as<uint32_t>();
    kp.cw = s->cw.as<uint32_t>(); kp.scene_idx = s->scene_idx.as<uint32_t>();
    kp.aos = s->caos.as<uint4>();
    kp.keys_out = s->keys.as<int32_t>();
    if (pl.Rs > 0) s->frame_index ^= 1u;       // this sort's frame was reset by the previous sort's first kernel (or at create)
    kp.frame = s->frame.as<SortFrame>() + s->frame_index;
    kp.next_frame = s->frame.as<SortFrame>() + (s->frame_index ^ 1u);
    kp.digit_total = s->radix.digit_total.as<uint32_t>();
    kp.sort_start = pl.sort_start;
    kp.render_count = pl.R;
    kp.last_splat = pl.last_splat;
    kp.im0 = c.im[0]; kp.im1 = c.im[1]; kp.im2 = c.im[2];
    kp.fm0 = mvp[2]; kp.fm1 = mvp[6]; kp.fm2 = mvp[10];
    if (pl.cull) {
        GS_TRY(s->keep_mask.ensure(sorter_keep_mask_bytes(s->max_count)));   // the key kernel writes whole 256-position windows
        kp.keep = s->keep_mask.as<unsigned long long>();
        memcpy(kp.mvp, mvp, sizeof(kp.mvp));
    }
    kp.count_dev = c.list_count_dev;
    return GS_OK;
}

// 3a. copy + keys (+ keep bits) of a planned gather in one kernel over leaf-major copies of the centres and payloads
static int launch_tree_front(gs_sorter* s, const SortCall& c, const SortPlan& pl, const KeyParams& kp) {
    gs_context* ctx = s->ctx;
    hipStream_t st = s->stream;
    TreeCopyParams cp;
    gs_tree_view(s->handover.tree->owner, &cp.v);
    const void* mesh_key = c.map ? (const void*)s->bound_mesh : nullptr;
    const uint32_t layout = c.map ? s->bound_mesh->layout_version : 0u;
    GS_TRY(s->pay_in.ensure((size_t)s->max_count * 4));
    if (s->leaf_cache_tree != cp.v.tree_uid || s->leaf_cache_centers != s->centers_version || s->leaf_cache_mesh != mesh_key ||
        s->leaf_cache_layout != layout || s->leaf_cache_uploaded != s->uploaded || !s->leaf_centers.p) {
        GS_TRY(s->leaf_centers.ensure((size_t)cp.v.tree_splats * 16 + 16));
        GS_TRY(s->leaf_pos.ensure((size_t)cp.v.tree_splats * 4 + 16));
        if (cp.v.tree_splats)
            hipLaunchKernelGGL(k_tree_leaf_cache, dim3(grid_for(cp.v.tree_splats, 1024, 4096)), dim3(256), 0, st, cp.v.leaf_indexes,
                               cp.v.tree_splats, s->caos.as<uint4>(), c.map, kp.last_splat, s->leaf_centers.as<uint4>(),
                               s->leaf_pos.as<uint32_t>());
        s->leaf_cache_tree = cp.v.tree_uid; s->leaf_cache_centers = s->centers_version; s->leaf_cache_mesh = mesh_key;
        s->leaf_cache_layout = layout; s->leaf_cache_uploaded = s->uploaded;
    }
    cp.leaf_centers = s->leaf_centers.as<uint4>();
    cp.leaf_pos = s->leaf_pos.as<uint32_t>();
    cp.idx_out = s->idx_in.as<uint32_t>();
    cp.pay_out = s->pay_in.as<uint32_t>();
    // (a workgroup ends with one atomic on the sort's kept counter, and same-address atomics retire at ~12 ns each:
    // 6.5 k workgroups queue ~80 us of them behind 30 us of memory traffic - eight workgroups per CU walk the leaves)
    const uint32_t cgrid = grid_for(cp.v.leaves, 4, (uint32_t)ctx->cu_count * 8u);
    if (pl.front == SORT_FRONT_TREE_CULL) hipLaunchKernelGGL(k_tree_copy_keys<true>, dim3(cgrid), dim3(256), 0, st, cp, kp);
    else hipLaunchKernelGGL(k_tree_copy_keys<false>, dim3(cgrid), dim3(256), 0, st, cp, kp);
    handover_copied(s->handover);
    return GS_OK;
}

// 3b. the visibility cull: compact, then sort the survivors (see k_minmax_count) - the list is what the bound mesh's vertex
// stage kept.  Leaves the list's length on the device (kp.count_dev) and min / max in the frame (kp.ext_minmax).
static int launch_vis_cull_front(gs_sorter* s, const SortCall& c, const SortPlan& pl, KeyParams& kp) {
    hipStream_t st = s->stream;
    gs_mesh* mesh = s->bound_mesh;
    ProjSet& ps = mesh->set();                              // the set the pending gs_mesh_project wrote
    const uint32_t R = pl.R;
    const bool stream = pl.front == SORT_FRONT_VIS_STREAM, lazy = pl.vis_derive != 0u;
    // a dynamic-mode sorter: the DYN instances key from five planes and the rows sort_stage_inputs stored on this stream (kp.rows)
    const bool dynamic = (kp.mode & MODE_DYNAMIC) != 0u;
    GS_TRY(s->idx_in.ensure((size_t)s->max_count * 4));
    GS_TRY(s->mask_copy.ensure(((size_t)s->max_count + 31) / 32 * 4 + 64));
    uint32_t* mask = ps.vis_orig.as<uint32_t>();
    // The projection left the by-original-index mask to us (gs_mesh_project of a full frame for a mesh whose bound sorter
    // culls by visibility): k_mask_derive_count builds it from the storage-order mask through the payload map.
    GS_REQUIRE(!lazy || c.map, "the pending projection expects the sorter to derive its visibility mask, but the sorter has no position map of the mesh");
    if (!stream) handover_list_overwritten(s->handover);    // k_mask_compact writes idx_in
    GS_TRY(s->chunk_counts.ensure((size_t)pl.counts_words * 4));
    if (stream) GS_TRY(s->pay_in.ensure((size_t)s->max_count * 4));
    uint32_t* counts = s->chunk_counts.as<uint32_t>();
    // (a forced compact front end derives the mask first as well: its counts are redone by k_minmax_count)
    if (lazy) hipLaunchKernelGGL(k_mask_derive_count, dim3(pl.derive_grid * VC_DERIVE_SUBS), dim3(VC_THREADS), 0, st, kp, c.map,
                                 ps.vis_mask.as<unsigned long long>(), ps.block_any.as<uint8_t>(), (mesh->uploaded + 255u) >> 8,
                                 pl.derive_len, VC_DERIVE_SUBS, reinterpret_cast<unsigned long long*>(mask), counts);
    if (stream) {
        if (!lazy) hipLaunchKernelGGL(k_mask_count, dim3(pl.front_grid), dim3(VC_THREADS), 0, st, kp, mask, pl.front_len, counts);
        auto* front = c.map ? (dynamic ? k_cull_front<true, true> : k_cull_front<true, false>)
                            : (dynamic ? k_cull_front<false, true> : k_cull_front<false, false>);
        hipLaunchKernelGGL(front, dim3(pl.front_grid), dim3(VC_THREADS), 0, st, kp, mask, s->mask_copy.as<uint32_t>(), counts, pl.front_len,
                           c.map, s->pay_in.as<uint32_t>(), lazy ? VC_DERIVE_SUBS : 1u);     // (lazy: only with a map, see above)
    } else {
        hipLaunchKernelGGL(dynamic ? k_minmax_count<true> : k_minmax_count<false>, dim3(pl.front_grid), dim3(VC_THREADS), 0, st, kp, mask,
                           pl.front_len, counts);
        hipLaunchKernelGGL(k_mask_compact, dim3(pl.front_grid), dim3(VC_THREADS), 0, st, mask, s->mask_copy.as<uint32_t>(), counts, R,
                           pl.front_len, s->idx_in.as<uint32_t>(), kp.frame);
    }
    // the mask is all zero again if this sort covered every splat the vertex stage looked at - and, where it derived the
    // mask itself, if the words beyond the ones it wrote were zero already (gs_mesh_project)
    if (R >= ps.vis_orig_count && (!lazy || ps.vis_orig_tail_zero)) ps.vis_orig_dirty = false;
    kp.idx_in = s->idx_in.as<uint32_t>();
    kp.count_dev = &kp.frame->kept;
    kp.ext_minmax = 1u;
    if (!stream) hipLaunchKernelGGL(k_depth_key<false>, dim3(pl.key_grid), dim3(256), 0, st, kp);
    return GS_OK;
}

// 3. the first kernel(s) of the sort: keys, min / max, the housekeeping (sort_begin) - one case per kernel family
static int launch_front_end(gs_sorter* s, const SortCall& c, const SortPlan& pl, KeyParams& kp) {
    hipStream_t st = s->stream;
    const dim3 grid(pl.front_grid);
    switch (pl.front) {
    case SORT_FRONT_KNOWN_WIDE: case SORT_FRONT_KNOWN_NARROW: case SORT_FRONT_KNOWN_COMPACT: {
        DepthLoaderArgs hl = {};
        hl.keys = s->keys.as<int32_t>(); hl.frame = kp.frame; hl.sort_start = 0u; hl.render_count = pl.R; hl.range = 1u << s->precision;
        hl.last_splat = kp.last_splat; hl.count_clamps = 1u;
        const dim3 hgrid(pl.pass[0].grid);                 // the kernel writes pass 0's histogram rows: one per workgroup of THAT grid
        uint32_t* group_rows = s->radix.digit_total.as<uint32_t>() + pl.pass0_slot * RADIX_SLOT_WORDS;
        uint32_t* bh = s->radix.block_hist.as<uint32_t>();
        CompactCentres cc = {};
        if (pl.front == SORT_FRONT_KNOWN_COMPACT) {
            cc.x = s->cx16.as<uint16_t>(); cc.y = s->cy16.as<uint16_t>(); cc.z = s->cz16.as<uint16_t>();
            cc.k0 = (uint32_t)s->c16_off[0] * (uint32_t)kp.im0 + (uint32_t)s->c16_off[1] * (uint32_t)kp.im1 +
                    (uint32_t)s->c16_off[2] * (uint32_t)kp.im2;         // static_key_int of the offset: uint32 wrap-around
            hipLaunchKernelGGL((k_depth_key_hist<true, true>), hgrid, dim3(HIST_THREADS), 0, st, kp, DepthLoader{hl}, pl.range_lo, pl.range_hi,
                               0, pl.pass0_slot, bh, group_rows, s->keys16.as<uint16_t>(), cc);
        } else if (pl.front == SORT_FRONT_KNOWN_NARROW) {
            hipLaunchKernelGGL(k_depth_key_hist<true>, hgrid, dim3(HIST_THREADS), 0, st, kp, DepthLoader{hl}, pl.range_lo, pl.range_hi, 0,
                               pl.pass0_slot, bh, group_rows, s->keys16.as<uint16_t>(), cc);
        } else {
            hipLaunchKernelGGL(k_depth_key_hist<false>, hgrid, dim3(HIST_THREADS), 0, st, kp, DepthLoader{hl}, pl.range_lo, pl.range_hi, 0,
                               pl.pass0_slot, bh, group_rows, (uint16_t*)nullptr, cc);
        }
        break;
    }
    case SORT_FRONT_TREE: case SORT_FRONT_TREE_CULL: GS_TRY(launch_tree_front(s, c, pl, kp)); break;
    case SORT_FRONT_VIS_STREAM: case SORT_FRONT_VIS_COMPACT: GS_TRY(launch_vis_cull_front(s, c, pl, kp)); break;
    case SORT_FRONT_CULL_VEC4: hipLaunchKernelGGL(k_depth_key_cull<true>, grid, dim3(256), 0, st, kp); break;
    case SORT_FRONT_CULL_IDX: hipLaunchKernelGGL(k_depth_key_cull<false>, grid, dim3(256), 0, st, kp); break;
    case SORT_FRONT_KEY_VEC4: hipLaunchKernelGGL(k_depth_key<true>, grid, dim3(256), 0, st, kp); break;
    case SORT_FRONT_KEY_IDX: hipLaunchKernelGGL(k_depth_key<false>, grid, dim3(256), 0, st, kp); break;
    default: GS_REQUIRE(false, "sort plan: unknown front end");
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// 4. the radix passes the plan lists
static int run_radix_passes(gs_sorter* s, const SortCall& c, const SortPlan& pl, const KeyParams& kp) {
    const RadixExec ex = {s->stream, &s->radix, s->ctx->lds_atomic_lane_order};
    PassBuffers b = {};
    b.dl.keys = s->keys.as<int32_t>();
    b.dl.keys16 = s->keys16.as<uint16_t>();
    b.dl.keep = pl.cull ? kp.keep : nullptr;
    b.dl.idx = pl.own_payloads ? s->pay_in.as<uint32_t>() : kp.idx_in;
    b.dl.map = pl.own_payloads ? nullptr : c.map;
    b.dl.frame = kp.frame;
    b.dl.sort_start = pl.sort_start;
    b.dl.render_count = pl.R;
    b.dl.range = 1u << s->precision;
    // (the loader clamps what it reads from `idx`: splat indexes normally, ready-made payloads after a fused copy / front end)
    b.dl.last_splat = pl.own_payloads ? pl.max_payload : kp.last_splat;
    b.dl.n_dev = pl.pass0_count == SORT_COUNT_KEPT ? &kp.frame->kept : pl.pass0_count == SORT_COUNT_LIST ? c.list_count_dev : nullptr;
    b.n_dev = pl.count_on_device ? &kp.frame->kept : nullptr;
    b.Rs = pl.Rs; b.val_bits = pl.val_bits;
    b.kbuf[0] = s->keyA.p; b.kbuf[1] = s->keyB.p;
    b.vbuf[0] = s->valA.as<uint32_t>(); b.vbuf[1] = s->valB.as<uint32_t>();
    b.out_tail = s->sorted.as<uint32_t>() + pl.sort_start;
    b.kept_out = pl.pass0_publishes ? &kp.frame->kept : nullptr;
    for (uint32_t p = 0; p < pl.passes; p++) GS_TRY(launch_pass(ex, pl.pass[p], p, b));
    return GS_OK;
}

// 5. the unsorted head, the result's bookkeeping, the optional host copy and statistics
static int sort_finish(gs_sorter* s, const SortCall& c, const SortPlanIn& in, const SortPlan& pl, const KeyParams& kp, uint32_t* sorted_out,
                       gs_sort_stats* stats) {
    hipStream_t st = s->stream;
    if (pl.sort_start > 0) {
        hipLaunchKernelGGL(k_copy_head, dim3(grid_for(pl.sort_start, 1024, 2048)), dim3(256), 0, st, kp.idx_in, c.map,
                           s->sorted.as<uint32_t>(), pl.sort_start, s->uploaded - 1u);
    }
    GS_HIP(hipGetLastError());
    if (s->timed_sort || st != s->ctx->stream) GS_HIP(hipEventRecord(s->ev1, st));   // a draw on another stream waits for it
    s->last_render = pl.R;
    s->last_sort = pl.Rs;
    s->last_passes = pl.passes;
    s->last_in = in;                           // what gs_sorter_debug_read (4, 5), the statistics and the draw read of this sort
    s->last_plan = pl;
    if (pl.Rs > 0) {                           // (a front end ran: `keys` holds this sort's depths, or it is stale from now on)
        s->keys_stale = pl.front == SORT_FRONT_KNOWN_NARROW || pl.front == SORT_FRONT_KNOWN_COMPACT;
        s->stale_im[0] = kp.im0; s->stale_im[1] = kp.im1; s->stale_im[2] = kp.im2;
        s->stale_count = pl.R;
    }
    s->result_frame = kp.frame;
    s->result_mesh = c.map ? s->bound_mesh : nullptr;
    s->result_unmap = c.unmap;
    s->result_payload_max = pl.max_payload;    // (the clamp of the host-visible un-mapping: payloads of a bound mesh are positions in ITS storage)
    s->has_result = true;

    uint32_t out_count = pl.R;
    if (sorted_out && pl.count_on_device) {        // the result's length is only known on the device
        SortFrame f;
        GS_HIP(hipMemcpyAsync(&f, kp.frame, sizeof(f), hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        out_count = f.kept;
    }
    if (sorted_out && out_count) {
        const void* src = s->sorted.p;
        if (c.unmap) {                             // the host always sees the caller's splat indexes
            GS_TRY(s->debug.ensure((size_t)s->max_count * 4));
            hipLaunchKernelGGL(k_unmap, dim3(grid_for(out_count, 1024, 2048)), dim3(256), 0, st, s->sorted.as<uint32_t>(), c.unmap,
                               s->debug.as<uint32_t>(), out_count, s->result_payload_max);
            GS_HIP(hipGetLastError());
            src = s->debug.p;
        }
        GS_HIP(hipMemcpyAsync(sorted_out, src, (size_t)out_count * 4, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
    }
    return stats ? sorter_collect_stats(s, stats) : GS_OK;
}

static int sorter_sort(gs_sorter* s, const float* mvp, const uint32_t* indexes_to_sort, bool device_list, uint32_t sort_count,
                       uint32_t render_count, const void* precomputed, const float* transforms, uint32_t* sorted_out,
                       gs_sort_stats* stats, const uint32_t* list_count_dev = nullptr) {
    GS_REQUIRE(s && mvp, "sorter / mvp == NULL");
    GS_REQUIRE_SCRATCH(s);
    SortCall c = {};
    c.mvp = mvp; c.indexes_to_sort = indexes_to_sort; c.device_list = device_list; c.precomputed = precomputed;
    c.transforms = transforms; c.list_count_dev = list_count_dev; c.sort_count = sort_count; c.render_count = render_count;
    SortPlanIn in;
    GS_TRY(sort_check(s, c, in));
    const SortPlan pl = plan_sort(in);
    KeyParams kp = {};
    ScopedDevice sd(s->ctx->device);
    GS_TRY(sort_stage_inputs(s, c, pl, kp));
    s->timed_sort = stats != nullptr || s->ctx->stage_events;
    if (s->timed_sort) GS_HIP(hipEventRecord(s->ev0, s->stream));
    s->clean_slot = pl.next_clean_slot;        // (unchanged when nothing is sorted)
    if (pl.front != SORT_FRONT_NONE) {
        GS_TRY(launch_front_end(s, c, pl, kp));
        GS_TRY(run_radix_passes(s, c, pl, kp));
    }
    return sort_finish(s, c, in, pl, kp, sorted_out, stats);
}

int gs_sorter_sort(gs_sorter* s, const float* mvp, const uint32_t* indexes_to_sort, uint32_t sort_count,
                   uint32_t render_count, const void* precomputed, const float* transforms, uint32_t* sorted_out,
                   gs_sort_stats* stats) {
    return sorter_sort(s, mvp, indexes_to_sort, false, sort_count, render_count, precomputed, transforms, sorted_out,
                            stats);
}

int gs_sorter_sort_gathered(gs_sorter* s, const float* mvp, uint32_t sort_count, const void* precomputed,
                            const float* transforms, uint32_t* sorted_out, gs_sort_stats* stats) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    const HandoverSort r = handover_sort_request(s->handover, sort_count);
    GS_REQUIRE(r.refused != HANDOVER_SORT_NO_LIST, "no gs_tree_gather has filled this sorter's index list");
    GS_REQUIRE(r.refused != HANDOVER_SORT_PARTIAL_ASYNC, "after an asynchronous gs_tree_gather only the whole list can be sorted: the "
                                                         "partial-sort schedule needs splatRenderCount on the host (pass render_count)");
    return sorter_sort(s, mvp, nullptr, true, r.sort_count, r.render_count, precomputed, transforms, sorted_out, stats,
                       r.count_on_device ? s->gathered_dev.as<uint32_t>() : nullptr);
}

// A bound sorter that culls by visibility and holds the mesh's position map derives the by-original-index mask itself
// (k_mask_derive_count): the mesh's next full-frame gs_mesh_project may then skip its per-survivor atomics.
static void sorter_tell_mesh(gs_sorter* s) {
    gs_mesh* m = s->bound_mesh;
    if (sorter_mesh_alive(s->ctx, m)) m->derive_orig_mask = s->visibility_cull && gs_mesh_payload_map(m, s->uploaded) != nullptr;
}

int gs_sorter_bind_mesh(gs_sorter* s, gs_mesh* m) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    GS_REQUIRE(!m || m->ctx == s->ctx, "mesh lives on another context");
    if (s->bound_mesh != m && sorter_mesh_alive(s->ctx, s->bound_mesh)) s->bound_mesh->derive_orig_mask = false;
    s->bound_mesh = m;
    sorter_tell_mesh(s);
    return GS_OK;
}

int gs_sorter_set_frustum_cull(gs_sorter* s, int enable) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    GS_REQUIRE(!enable || !(s->flags & GS_SORT_DYNAMIC), "the per-splat frustum cull is not available to a dynamic-mode sorter");
    s->frustum_cull = enable != 0;
    return GS_OK;
}

int gs_sorter_set_visibility_cull(gs_sorter* s, int enable) {
    GS_REQUIRE(s != nullptr, "sorter == NULL");
    s->visibility_cull = enable != 0;
    sorter_tell_mesh(s);
    return GS_OK;
}

int gs_sorter_last_stats(gs_sorter* s, gs_sort_stats* stats) {
    GS_REQUIRE(s && stats, "sorter / stats == NULL");
    GS_REQUIRE(s->has_result, "no sort has run");
    ScopedDevice sd(s->ctx->device);
    return sorter_collect_stats(s, stats);
}

int gs_sorter_debug_read(gs_sorter* s, int what, void* dst, uint32_t count) {
    GS_REQUIRE(s && dst, "sorter / dst == NULL");
    GS_REQUIRE(s->has_result, "no sort has run");
    const SortPlan& lp = s->last_plan;
    if (what == 4) {
        // the last sort's front end, host words: {1 = k_depth_key_hist with a known range, |extreme set| (0: none), lo, hi as the
        // host computed them (0, 0 on the other path), 1 = the set covers the current centres, pass 0's slot of group rows,
        // 1 = that front end stored 16-bit radix keys, 1 = it read the 16-bit centre planes}
        const bool valid = s->extreme_ok && s->extreme_version == s->centers_version;
        const bool compact = lp.front == SORT_FRONT_KNOWN_COMPACT, narrow = compact || lp.front == SORT_FRONT_KNOWN_NARROW;
        const int32_t w[8] = {lp.known_range ? 1 : 0, valid ? (int32_t)(s->extreme.size() / 4) : 0, lp.range_lo, lp.range_hi,
                              valid ? 1 : 0, (int32_t)lp.pass0_slot, narrow ? 1 : 0, compact ? 1 : 0};
        GS_REQUIRE(count <= 8u, "selector 4 holds 8 words");
        memcpy(dst, w, (size_t)count * 4);
        return GS_OK;
    }
    if (what == 5) {
        // the last sort's plan, host words: the SortPlanIn it was made from, then the SortPlan that ran (sort_plan.hpp)
        constexpr uint32_t IN_WORDS = sizeof(SortPlanIn) / 4, WORDS = IN_WORDS + sizeof(SortPlan) / 4;
        GS_REQUIRE(count <= WORDS, "selector 5 holds the words of SortPlanIn and SortPlan");
        uint32_t w[WORDS];
        memcpy(w, &s->last_in, sizeof(SortPlanIn));
        memcpy(w + IN_WORDS, &lp, sizeof(SortPlan));
        memcpy(dst, w, (size_t)count * 4);
        return GS_OK;
    }
    GS_REQUIRE(count <= s->last_render, "count exceeds the last render_count");
    ScopedDevice sd(s->ctx->device);
    hipStream_t st = s->stream;
    const void* src = nullptr;
    if (what == 0 || what == 1) GS_TRY(sorter_refresh_keys(s));     // (the depths of a sort that stored only 16-bit radix keys)
    if (what == 0) src = s->keys.p;
    else if (what == 2) {
        src = s->sorted.p;
        if (sorter_mesh_alive(s->ctx, s->result_mesh) && s->result_unmap && count) {
            GS_TRY(s->debug.ensure((size_t)s->max_count * 4));
            hipLaunchKernelGGL(k_unmap, dim3(grid_for(count, 1024, 2048)), dim3(256), 0, st, s->sorted.as<uint32_t>(),
                               s->result_unmap, s->debug.as<uint32_t>(), count, s->result_payload_max);
            GS_HIP(hipGetLastError());
            src = s->debug.p;
        }
    }
    else if (what == 1) {
        GS_TRY(s->debug.ensure((size_t)s->max_count * 4));
        DepthLoaderArgs dl = {};
        dl.keys = s->keys.as<int32_t>();
        dl.frame = s->frame.as<SortFrame>() + s->frame_index;
        dl.sort_start = s->last_render - s->last_sort;
        dl.render_count = s->last_render;
        dl.range = 1u << s->precision;
        GS_HIP(hipMemsetAsync(s->debug.p, 0, (size_t)s->last_render * 4, st));
        if (s->last_sort)
            hipLaunchKernelGGL(k_debug_buckets, dim3(grid_for(s->last_sort, 1024, 2048)), dim3(256), 0, st, DepthLoader{dl}, s->debug.as<int32_t>());
        GS_HIP(hipGetLastError());
        src = s->debug.p;
    } else if (what == 3) {
        GS_REQUIRE(lp.count_on_device, "the last sort did not cull");
        if (lp.vis_cull) {                  // the bound mesh's per-splat mask (original splat numbering), as consumed
            GS_REQUIRE((size_t)count * 4 <= s->mask_copy.bytes, "count exceeds the mask length");
            src = s->mask_copy.p;
        } else {
            GS_REQUIRE((size_t)count * 4 <= s->keep_mask.bytes, "count exceeds the mask length");
            src = s->keep_mask.p;
        }
    } else {
        GS_REQUIRE(false, "unknown debug selector");
    }
    if (count) GS_HIP(hipMemcpyAsync(dst, src, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

}  // extern "C"
