// distances.hip — SplatMesh.computeDistancesOnGPU (/root/reference/src/splatmesh/SplatMesh.js:1701-1814) on gfx950: the
// reference's transform-feedback vertex shader (:1449-1490), all four permutations, over every uploaded splat of a mesh.
// The result is one int32 / float per ORIGINAL splat index: what getBufferSubData hands to the sort worker as
// precomputedDistances (src/Viewer.js:1893-1936).  Built with -ffp-contract=off; the float paths also spell their
// arithmetic with non-contracting intrinsics (a GL driver may contract them, so the reference is defined to within an ulp
// there; this file fixes the order documented in include/gsplat_hip.h).
#include <math.h>

#include "gs_internal.hpp"

// Math.round((double)f * 1000.0) stored into an Int32Array (getIntegerCenters, SplatMesh.js:1912-1926), i.e. JS ToInt32:
// NaN / +-Infinity -> 0, everything else wraps modulo 2^32.  The fp32 * 1000 product is exact in fp64 (24 + 7 significant
// bits).  Math.round is "nearest, halves up": floor(t) + (t - floor(t) >= 0.5) - t - floor(t) is exact, whereas the naive
// floor(t + 0.5) rounds the sum itself once |t| >= 2^52.  The reduction r - 2^32 * floor(r / 2^32) is exact too: the scaling
// is by a power of two and the difference is an integer below 2^32, which fp64 represents.
__host__ __device__ inline uint32_t js_round1000_int32(float f) {
    const double t = (double)f * 1000.0;
    if (!(t - t == 0.0)) return 0u;                                   // NaN, +-Infinity
    double r = floor(t);
    if (t - r >= 0.5) r += 1.0;
    const double m = r - 4294967296.0 * floor(r * (1.0 / 4294967296.0));
    return (uint32_t)m;
}

// Per-scene rows of the shader's uniforms: integer {x, y, z, w} (static: the ivec3 modelViewProj in scene 0, w unused) and
// float {T[2], T[6], T[10], T[14]} (static: the vec3 in scene 0).  Rows of scenes beyond scene_count are zero, as GL leaves
// uniforms nobody set.
struct DistRows {
    uint32_t iu[GS_MAX_SCENES][4];
    float fu[GS_MAX_SCENES][4];
};

// A thread per storage position p reads the mesh's planes coalesced and writes out[inv_perm[p]]: a 4-byte write at random for a
// Morton-ordered mesh (map = inv_perm), a coalesced one for a GS_MESH_KEEP_ORDER mesh (map = nullptr).  The other scheme - a
// thread per original index gathering its centre through perm, three 4-byte reads at random and a coalesced write - measured 3.8x
// slower at 5.8 M Morton-ordered splats (305 us against 80 us, static integer).
template <bool INTEGER, bool DYNAMIC>
__global__ __launch_bounds__(256) void k_distances(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                   const uint32_t* __restrict__ scene_idx, const uint32_t* __restrict__ map,
                                                   uint32_t count, DistRows rows, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_rows[GS_MAX_SCENES][4];                     // the row of THIS permutation (integer or float bits)
    if (DYNAMIC) {
        for (uint32_t t = threadIdx.x; t < GS_MAX_SCENES * 4; t += blockDim.x)
            s_rows[t >> 2][t & 3] = INTEGER ? rows.iu[t >> 2][t & 3] : __float_as_uint(rows.fu[t >> 2][t & 3]);
        __syncthreads();
    }
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < count; p += stride) {
        const float fx = px[p], fy = py[p], fz = pz[p];
        const uint32_t sc = DYNAMIC && scene_idx ? (scene_idx[p] & (GS_MAX_SCENES - 1u)) : 0u;
        uint32_t d;
        if (INTEGER) {
            // ivec4 center = getIntegerCenters(padFour): x, y, z as above, w = 1000; GLSL ES 3.00 int arithmetic wraps
            const uint32_t x = js_round1000_int32(fx), y = js_round1000_int32(fy), z = js_round1000_int32(fz);
            if (DYNAMIC) {
                const uint32_t* r = s_rows[sc];                        // center.x * t.x + center.y * t.y + center.z * t.z + t.w * center.w
                d = x * r[0] + y * r[1] + z * r[2] + r[3] * 1000u;
            } else {                                                   // center.x * m.x + center.y * m.y + center.z * m.z
                d = x * rows.iu[0][0] + y * rows.iu[0][1] + z * rows.iu[0][2];
            }
        } else {
            float s;
            if (DYNAMIC) {                                             // (transforms[sceneIndex] * vec4(center.xyz, 1.0)).z
                const uint32_t* r = s_rows[sc];
                s = __fmul_rn(__uint_as_float(r[0]), fx);
                s = __fadd_rn(s, __fmul_rn(__uint_as_float(r[1]), fy));
                s = __fadd_rn(s, __fmul_rn(__uint_as_float(r[2]), fz));
                s = __fadd_rn(s, __uint_as_float(r[3]));
            } else {                                                   // center.x * m.x + center.y * m.y + center.z * m.z
                s = __fmul_rn(fx, rows.fu[0][0]);
                s = __fadd_rn(s, __fmul_rn(fy, rows.fu[0][1]));
                s = __fadd_rn(s, __fmul_rn(fz, rows.fu[0][2]));
            }
            d = __float_as_uint(s);
        }
        out[map ? map[p] : p] = d;
    }
}

template <bool INTEGER, bool DYNAMIC>
static void launch_distances(dim3 g, hipStream_t st, const gs_mesh* m, const uint32_t* map, uint32_t n, const DistRows& rows,
                             uint32_t* out) {
    hipLaunchKernelGGL((k_distances<INTEGER, DYNAMIC>), g, dim3(256), 0, st, m->px.as<float>(), m->py.as<float>(), m->pz.as<float>(),
                       DYNAMIC ? m->scene_idx.as<uint32_t>() : nullptr, map, n, rows, out);
}

extern "C" {

int gs_mesh_compute_distances(gs_mesh* m, uint32_t flags, const void* uniforms, uint32_t scene_count, void* out_host,
                              gs_sorter* dst) {
    GS_REQUIRE(m && uniforms, "mesh / uniforms == NULL");
    GS_REQUIRE((flags & ~(GS_SORT_INTEGER | GS_SORT_DYNAMIC)) == 0, "unknown distance flags (GS_SORT_INTEGER | GS_SORT_DYNAMIC)");
    GS_REQUIRE(scene_count >= 1 && scene_count <= GS_MAX_SCENES, "scene_count outside 1..GS_MAX_SCENES");
    const bool integer = (flags & GS_SORT_INTEGER) != 0, dynamic = (flags & GS_SORT_DYNAMIC) != 0;
    GS_REQUIRE(!dynamic || scene_count == 1 || m->scene_idx.p, "several scenes but no scene indexes uploaded (gs_mesh_upload_scene_indexes)");
    GS_REQUIRE(!dst || dst->ctx == m->ctx, "the sorter lives on another context");
    const uint32_t n = m->uploaded;
    GS_REQUIRE(!dst || dst->max_count >= n, "the sorter holds fewer splats than the mesh has uploaded");
    gs_context* ctx = m->ctx;
    ScopedDevice sd(ctx->device);
    hipStream_t st = ctx->stream;

    DistRows rows = {};
    if (integer) {
        const int32_t* u = (const int32_t*)uniforms;
        for (uint32_t s = 0; s < (dynamic ? scene_count : 1u); s++)
            for (uint32_t k = 0; k < (dynamic ? 4u : 3u); k++) rows.iu[s][k] = (uint32_t)u[(dynamic ? 4u : 3u) * s + k];
    } else if (dynamic) {
        const float* u = (const float*)uniforms;
        for (uint32_t s = 0; s < scene_count; s++)
            for (uint32_t k = 0; k < 4; k++) rows.fu[s][k] = u[16 * s + 4 * k + 2];       // row 2 of a column-major mat4
    } else {
        const float* u = (const float*)uniforms;
        for (uint32_t k = 0; k < 3; k++) rows.fu[0][k] = u[k];
    }

    uint32_t* out;
    if (dst) {
        GS_TRY(dst->precomputed.ensure((size_t)dst->max_count * 4));   // the size gs_sorter_sort gives it: never re-allocated there
        out = dst->precomputed.as<uint32_t>();
        if (dst->stream != st) {                                       // sorts still reading the buffer finish first
            GS_HIP(hipEventRecord(dst->ev_handover, dst->stream));
            GS_HIP(hipStreamWaitEvent(st, dst->ev_handover, 0));
        }
    } else {
        GS_TRY(m->distances.ensure((size_t)m->max_count * 4));
        out = m->distances.as<uint32_t>();
    }
    if (n) {
        const uint32_t* map = m->reorder ? m->inv_perm.as<uint32_t>() : nullptr;   // storage position -> original index
        uint32_t blocks = (n + 255u) / 256u, cap = (uint32_t)ctx->cu_count * 8u;
        const dim3 g(blocks < cap ? blocks : cap);
        if (integer && dynamic) launch_distances<true, true>(g, st, m, map, n, rows, out);
        else if (integer) launch_distances<true, false>(g, st, m, map, n, rows, out);
        else if (dynamic) launch_distances<false, true>(g, st, m, map, n, rows, out);
        else launch_distances<false, false>(g, st, m, map, n, rows, out);
        GS_HIP(hipGetLastError());
    }
    if (dst) {
        if (dst->stream != st) {                                       // the sorter's next sort reads what this wrote
            GS_HIP(hipEventRecord(dst->ev_handover, st));
            GS_HIP(hipStreamWaitEvent(dst->stream, dst->ev_handover, 0));
        }
        dst->dev_distances = true;
        dst->dev_distances_count = n;
        dst->dev_distances_integer = integer;
    }
    if (out_host) {
        if (n) GS_HIP(hipMemcpyAsync(out_host, out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
    }
    return GS_OK;
}

}  // extern "C"
