// bounds.hip — gs_mesh_bounds: where a range of the mesh's splats is, reduced on the device from the planes the mesh keeps.
//
// The reference walks every centre on the host: SplatMesh.updateVisibleRegion (src/splatmesh/SplatMesh.js:1172-1199) for the
// largest distance from the averaged scene centre - what drives the scene fade-in (GS_CAM_FADE_IN) - and
// SplatMesh.computeBoundingBox (:2066-2095) for the box.  Since assets are decoded on the device (gs_mesh_upload_asset) no host
// copy of the centres exists here, so both come from ONE pass over px / py / pz (+ inv_perm, scene_idx).  The kernel only reads:
// no plane of the mesh, no draw state and no other kernel is touched.
#include <algorithm>
#include <math.h>
#include <vector>

#include "gs_internal.hpp"

namespace {

// One per workgroup.  Minimum and maximum are exact, so the joined result does not depend on the grid.
struct BoundsPartial {
    float mn[3], mx[3];
    uint32_t n, pad;
    double d;                          // max |c - center|^2, >= 0
};
constexpr uint32_t BOUNDS_MAX_BLOCKS = 1024;
constexpr size_t BOUNDS_TRANSFORMS_OFF = sizeof(BoundsPartial) * BOUNDS_MAX_BLOCKS;   // double [16 * GS_MAX_SCENES] behind the partials

struct BoundsArgs {
    const float *px, *py, *pz;
    const uint32_t* inv_perm;          // storage position -> original splat index; NULL: the mesh keeps upload order
    const uint32_t* scene_idx;         // per storage position; NULL: every splat is scene 0
    const double* transforms;          // column-major 4x4 per scene; NULL: centres as stored
    uint32_t pos_begin, pos_end;       // storage positions to walk: the slotted range that holds [from, from + count)
    uint32_t from, count, scene_count;
    double cx, cy, cz;
};

__device__ __forceinline__ void bounds_join(BoundsPartial& a, const BoundsPartial& b) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (b.mn[k] < a.mn[k]) a.mn[k] = b.mn[k];
        if (b.mx[k] > a.mx[k]) a.mx[k] = b.mx[k];
    }
    if (b.d > a.d) a.d = b.d;
    a.n += b.n;
}

// Every product and sum below is one fp64 operation, rounded on its own, in the order three.js writes them
// (Vector3.applyMatrix4, Vector3.sub, Vector3.length without the root): this file is built with -ffp-contract=off.
__global__ __launch_bounds__(256) void k_bounds(const BoundsArgs a, BoundsPartial* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ BoundsPartial s_part[4];
    BoundsPartial p;
#pragma unroll
    for (int k = 0; k < 3; k++) { p.mn[k] = INFINITY; p.mx[k] = -INFINITY; }
    p.n = 0u; p.pad = 0u; p.d = 0.0;
    const uint32_t span = a.pos_end - a.pos_begin;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < span; i += gridDim.x * blockDim.x) {
        const uint32_t pos = a.pos_begin + i;                 // < pos_end <= uploaded
        const uint32_t orig = a.inv_perm ? a.inv_perm[pos] : pos;
        if (orig - a.from >= a.count) continue;               // (unsigned: also drops orig < from)
        double x = (double)a.px[pos], y = (double)a.py[pos], z = (double)a.pz[pos];
        float bx = a.px[pos], by = a.py[pos], bz = a.pz[pos];
        if (a.transforms) {
            uint32_t s = a.scene_idx ? a.scene_idx[pos] : 0u;
            if (s >= a.scene_count) s = 0u;
            const double* e = a.transforms + 16u * s;
            const double w = 1.0 / (e[3] * x + e[7] * y + e[11] * z + e[15]);
            const double tx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w;
            const double ty = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w;
            const double tz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w;
            x = tx; y = ty; z = tz;
            bx = (float)x; by = (float)y; bz = (float)z;      // the Float32Array store of fillSplatCenterArray
        }
        if (x != x || y != y || z != z) continue;             // a NaN component: the splat takes part in nothing
        if (bx < p.mn[0]) p.mn[0] = bx;
        if (by < p.mn[1]) p.mn[1] = by;
        if (bz < p.mn[2]) p.mn[2] = bz;
        if (bx > p.mx[0]) p.mx[0] = bx;
        if (by > p.mx[1]) p.mx[1] = by;
        if (bz > p.mx[2]) p.mx[2] = bz;
        const double dx = x - a.cx, dy = y - a.cy, dz = z - a.cz;
        const double d = dx * dx + dy * dy + dz * dz;
        if (d > p.d) p.d = d;
        p.n++;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        BoundsPartial q;
#pragma unroll
        for (int k = 0; k < 3; k++) { q.mn[k] = __shfl_xor(p.mn[k], o, 64); q.mx[k] = __shfl_xor(p.mx[k], o, 64); }
        q.d = __shfl_xor(p.d, o, 64);
        q.n = __shfl_xor(p.n, o, 64);
        bounds_join(p, q);
    }
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < 4; w++) bounds_join(p, s_part[w]);
        out[blockIdx.x] = p;
    }
}

}  // namespace

extern "C" int gs_mesh_bounds(gs_mesh* m, uint32_t from, uint32_t count, const double* center, const double* transforms,
                              uint32_t scene_count, uint32_t flags, gs_bounds* out) {
    GS_REQUIRE(m && center && out, "mesh / center / out == NULL");
    GS_REQUIRE((flags & ~GS_BOUNDS_TRANSFORM) == 0u, "unknown flags");
    const bool transform = (flags & GS_BOUNDS_TRANSFORM) != 0u;
    GS_REQUIRE(!transform || (transforms && scene_count >= 1u && scene_count <= GS_MAX_SCENES),
               "GS_BOUNDS_TRANSFORM needs transforms of 1..GS_MAX_SCENES scenes");
    gs_bounds r;
    memset(&r, 0, sizeof(r));
    if (count == 0u) {
        *out = r;
        return GS_OK;
    }
    // the slotted range that holds the whole of [from, from + count): a fresh segment is stored in its own slots, so the splats
    // of a slotted range occupy exactly the storage positions of that range
    uint32_t pos_begin = 0u, pos_end = 0u;
    if (const SlotRange* s = m->slotted.holding(from, count)) { pos_begin = s->begin; pos_end = s->end; }
    GS_REQUIRE(pos_end > pos_begin && pos_end <= m->uploaded && pos_end <= m->max_count, "the range is not wholly uploaded");
    ScopedDevice sd(m->ctx->device);
    hipStream_t st = m->ctx->stream;
    GS_TRY(m->bounds_buf.ensure(BOUNDS_TRANSFORMS_OFF + sizeof(double) * 16 * GS_MAX_SCENES));
    char* buf = m->bounds_buf.as<char>();
    BoundsArgs a;
    a.px = m->px.as<float>(); a.py = m->py.as<float>(); a.pz = m->pz.as<float>();
    a.inv_perm = m->reorder ? m->inv_perm.as<uint32_t>() : nullptr;
    a.scene_idx = m->scene_idx.as<uint32_t>();
    a.transforms = nullptr;
    a.pos_begin = pos_begin; a.pos_end = pos_end;
    a.from = from; a.count = count; a.scene_count = scene_count;
    a.cx = center[0]; a.cy = center[1]; a.cz = center[2];
    if (transform) {
        GS_HIP(hipMemcpyAsync(buf + BOUNDS_TRANSFORMS_OFF, transforms, sizeof(double) * 16 * scene_count, hipMemcpyHostToDevice, st));
        a.transforms = reinterpret_cast<const double*>(buf + BOUNDS_TRANSFORMS_OFF);
    }
    // a few workgroups per compute unit, each striding over the positions; no workgroup waits for another
    const uint32_t want = (pos_end - pos_begin + 255u) / 256u;
    const uint32_t cap = std::min<uint32_t>(BOUNDS_MAX_BLOCKS, (uint32_t)std::max(m->ctx->cu_count, 1) * 4u);
    const uint32_t blocks = std::min(want, cap);
    hipLaunchKernelGGL(k_bounds, dim3(blocks), dim3(256), 0, st, a, reinterpret_cast<BoundsPartial*>(buf));
    GS_HIP(hipGetLastError());
    std::vector<BoundsPartial> part(blocks);
    GS_HIP(hipMemcpyAsync(part.data(), buf, sizeof(BoundsPartial) * blocks, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const BoundsPartial& p : part) {                     // in workgroup order
        for (int k = 0; k < 3; k++) {
            if (p.mn[k] < mn[k]) mn[k] = p.mn[k];
            if (p.mx[k] > mx[k]) mx[k] = p.mx[k];
        }
        if (p.d > r.max_dist_sq) r.max_dist_sq = p.d;
        r.count += p.n;
    }
    if (r.count)
        for (int k = 0; k < 3; k++) { r.box_min[k] = mn[k]; r.box_max[k] = mx[k]; }
    *out = r;
    return GS_OK;
}
