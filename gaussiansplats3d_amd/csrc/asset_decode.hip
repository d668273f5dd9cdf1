// asset_decode.hip — the per-splat decode of an opened asset on the device: file rows -> the staging layout a
// mesh upload commits (gs_mesh_upload_asset) and the sorter's `centers` message (gs_sorter_upload_asset_centers).
// The kernels take a ROW SOURCE (a template parameter, as XF is one): the .ksplat image (also an INRIA-v1 PLY's level-0
// image; KsplatSource, the reader the host fill uses too), the 32-byte rows of a .splat, the 16-byte vertex rows + chunk rows +
// SH bytes of a PlayCanvas compressed PLY, the six byte planes of an inflated .spz, or the index rows + decoded codebook of an INRIA-v2
// PLY, or the trainer's own rows of a streamed INRIA-v1 PLY.  The last five produce the level-0 tuple in registers through asset_internal.hpp's row arithmetic - the functions the host's image builder calls - so only file rows
// cross the bus and the level-0 image is never built on this path.
// What a thread does with its row is asset_fill_splat (asset_internal.hpp): the one body gs_asset_fill (assets.hip) loops over,
// compiled for both sides, so the planes are bit-equal to what gs_asset_fill + gs_mesh_upload (+ gs_mesh_upload_sh_u8) leave.
// This file keeps what only the decode has: the launches (the sources over file rows and the staging of a range are
// asset_sources.hpp, shared with the .ksplat encoder), and
//   integer centres              src/splatmesh/SplatMesh.js:1912-1948
// Header and section parsing stay host code (assets.hip); the device sees a section table and searches it per splat.
#include "asset_sources.hpp"

namespace {

struct NoTransform { uint32_t none; };   // the untransformed instantiations carry no matrix in their kernel argument
struct DevTransform {          // the transformed ones: 16 + 9 + 25 doubles and the file's 8-bit SH range, by value
    AssetTransform t;
    double sh_min, sh_max;
};
__device__ __forceinline__ const AssetTransform& transform_of(const DevTransform& x) { return x.t; }
__device__ __forceinline__ AssetTransform transform_of(const NoTransform&) { return AssetTransform(); }   // never read
__device__ __forceinline__ double sh_lo(const DevTransform& x) { return x.sh_min; }
__device__ __forceinline__ double sh_hi(const DevTransform& x) { return x.sh_max; }
__device__ __forceinline__ double sh_lo(const NoTransform&) { return 0.0; }
__device__ __forceinline__ double sh_hi(const NoTransform&) { return 0.0; }

// One thread per splat: asset splat first + i -> element i of the staging arrays (MeshStaging).
// SURFEL: into a GS_MESH_SURFEL mesh - the covariance slot receives (sx, sy, 1, qx, qy, qz) (asset_fill_splat)
template <class Source, bool XF, class Transform, bool SURFEL = false>
__global__ __launch_bounds__(256) void k_asset_decode(Source v, Transform xf, uint32_t first, uint32_t count, uint32_t min_alpha,
                                                      float* __restrict__ centers, float* __restrict__ cov_f32,
                                                      uint16_t* __restrict__ cov_f16, uint32_t* __restrict__ rgba,
                                                      uint16_t* __restrict__ sh_f16, uint8_t* __restrict__ sh_u8) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if constexpr (LdsTable<Source>::floats != 0) {          // before any thread leaves: the last workgroup's spare threads copy and wait too
        __shared__ __align__(16) float table[LdsTable<Source>::floats];
        v.load_table(table);
    }
    if (i >= count) return;
    asset_fill_splat<XF, false, SURFEL>(v.row(first + i), transform_of(xf), v.sh_degree, v.ncomp, sh_lo(xf), sh_hi(xf), min_alpha, i, centers,
                                cov_f32, cov_f16, rgba, sh_f16, sh_u8, nullptr, nullptr);
}

// The sorter's `centers` message of asset splats [first, first + count): padFour AoS, written where a copy from the host would
// have put it.  integer: Math.round(fp32 centre * 1000.0) as util.integer_centers pins it - floor(v + 0.5) in double - with
// w = 1000; a NaN or a value outside int32 becomes INT32_MIN (what the host's double -> int32 conversion stores).  Else the float
// centre with w = 1.0.
template <class Source, bool XF, class Transform>
__global__ __launch_bounds__(256) void k_asset_centers(Source v, Transform xf, uint32_t first, uint32_t count, int integer,
                                                       uint4* __restrict__ aos) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    double d[3];
    float c[3];
    v.centre(first + i, d);
    store_centre<XF>(transform_of(xf), d, c);
    uint32_t o[3];
    for (int k = 0; k < 3; k++) {
        if (integer) {
            const double r = floor((double)c[k] * 1000.0 + 0.5);
            o[k] = (r >= -2147483648.0 && r < 2147483648.0) ? (uint32_t)(int32_t)r : 0x80000000u;
        } else {
            o[k] = __builtin_bit_cast(uint32_t, c[k]);
        }
    }
    aos[i] = make_uint4(o[0], o[1], o[2], integer ? 1000u : __builtin_bit_cast(uint32_t, 1.0f));
}

// gs_mesh_upload_asset's source: a segment of the staging is filled by k_asset_decode
DevTransform dev_transform(const gs_asset* a) { return DevTransform{a->xf, a->sh_min, a->sh_max}; }

template <class Source>
struct AssetRows : MeshUploadSource {
    Source view;
    const gs_asset* asset;
    uint32_t first, min_alpha;
    int fill(gs_mesh* m, uint32_t o, uint32_t count, const MeshStaging& s, hipStream_t st) override {
        const bool half = (m->flags & GS_MESH_COV_HALF) != 0;
        const dim3 grid((count + 255u) / 256u), block(256);
        float* cov32 = half ? nullptr : (float*)(s.base + s.off_cov);
        uint16_t* cov16 = half ? (uint16_t*)(s.base + s.off_cov) : nullptr;
        uint16_t* sh16 = s.sh_u8 ? nullptr : (uint16_t*)(s.base + s.off_sh);
        uint8_t* sh8 = s.sh_u8 ? (uint8_t*)(s.base + s.off_sh) : nullptr;
        if (m->flags & GS_MESH_SURFEL)                     // (never with a transform: gs_mesh_upload_asset refuses that)
            hipLaunchKernelGGL((k_asset_decode<Source, false, NoTransform, true>), grid, block, 0, st, view, NoTransform{0u}, first + o, count,
                               min_alpha, (float*)s.base, cov32, cov16, (uint32_t*)(s.base + s.off_rgba), sh16, sh8);
        else if (asset->has_transform)
            hipLaunchKernelGGL((k_asset_decode<Source, true, DevTransform>), grid, block, 0, st, view, dev_transform(asset), first + o, count,
                               min_alpha, (float*)s.base, cov32, cov16, (uint32_t*)(s.base + s.off_rgba), sh16, sh8);
        else
            hipLaunchKernelGGL((k_asset_decode<Source, false, NoTransform>), grid, block, 0, st, view, NoTransform{0u}, first + o, count,
                               min_alpha, (float*)s.base, cov32, cov16, (uint32_t*)(s.base + s.off_rgba), sh16, sh8);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
};

template <class Source>
int mesh_upload_rows(gs_mesh* m, uint32_t from, gs_asset* a, uint32_t first, uint32_t count, uint32_t min_alpha, bool mesh_u8) {
    AssetRows<Source> src;
    GS_TRY(asset_stage(a, first, count, m->asset_dev, m->ctx->stream, &src.view, false));
    src.asset = a;
    src.first = first;
    src.min_alpha = min_alpha;
    src.stages_sh_u8 = mesh_u8;
    return gs_mesh_upload_from(m, from, count, src);
}

template <class Source>
int sorter_upload_rows(gs_sorter* s, uint32_t from, gs_asset* a, uint32_t first, uint32_t count) {
    Source view;
    GS_TRY(asset_stage(a, first, count, s->asset_dev, s->stream, &view, true));
    const dim3 grid((count + 255u) / 256u), block(256);
    const int integer = (s->flags & GS_SORT_INTEGER) ? 1 : 0;
    if (a->has_transform)
        hipLaunchKernelGGL((k_asset_centers<Source, true, DevTransform>), grid, block, 0, s->stream, view, dev_transform(a), first, count,
                           integer, s->caos.as<uint4>() + from);
    else
        hipLaunchKernelGGL((k_asset_centers<Source, false, NoTransform>), grid, block, 0, s->stream, view, NoTransform{0u}, first, count,
                           integer, s->caos.as<uint4>() + from);
    GS_HIP(hipGetLastError());
    return GS_OK;
}


}  // namespace

extern "C" {

int gs_mesh_upload_asset(gs_mesh* m, uint32_t from, gs_asset* a, uint32_t first, uint32_t count, uint32_t min_alpha) {
    GS_REQUIRE(m && a, "mesh / asset == NULL");
    GS_REQUIRE((uint64_t)from + count <= m->max_count, "range exceeds max_splat_count");
    GS_REQUIRE((uint64_t)first + count <= a->ready(), a->stream ? "range exceeds the stream's ready splats (gs_asset_stream_info.splats_ready)"
                                                                 : "range exceeds the asset's splat count");
    GS_REQUIRE(m->sh_degree == a->sh_degree, "the mesh's SH degree differs from the asset's (gs_asset_info.sh_degree)");
    const bool mesh_u8 = (m->flags & GS_MESH_SH_U8) != 0;
    GS_REQUIRE(m->sh_degree == 0 || mesh_u8 == (a->level == 2),
               "GS_MESH_SH_U8 must be set exactly for a file whose SH are uint8 (gs_asset_info.sh_level == 2)");
    GS_REQUIRE(!((m->flags & GS_MESH_SURFEL) && a->has_transform),
               "a GS_MESH_SURFEL mesh takes untransformed scales and rotations: the asset has a scene transform (gs_asset_set_transform)");
    if (count == 0) return GS_OK;
    ScopedDevice sd(m->ctx->device);
    // (an earlier call's decode kernels have finished: every upload synchronises before it returns)
    return with_source_of(a, [&](auto source) {
        return mesh_upload_rows<typename decltype(source)::type>(m, from, a, first, count, min_alpha, mesh_u8);
    });
}

int gs_sorter_upload_asset_centers(gs_sorter* s, uint32_t from, gs_asset* a, uint32_t first, uint32_t count,
                                   const uint32_t* scene_indexes) {
    GS_REQUIRE(s && a, "sorter / asset == NULL");
    GS_REQUIRE((uint64_t)from + count <= s->max_count, "range exceeds max_splat_count");
    GS_REQUIRE((uint64_t)first + count <= a->ready(), a->stream ? "range exceeds the stream's ready splats (gs_asset_stream_info.splats_ready)"
                                                                 : "range exceeds the asset's splat count");
    GS_REQUIRE(!(s->flags & GS_SORT_DYNAMIC) || scene_indexes, "dynamic sorter needs scene_indexes");
    GS_REQUIRE(!(s->flags & GS_SORT_DYNAMIC) || !a->has_transform,
               "a dynamic sorter takes untransformed centres: dynamic mode applies scene transforms per frame and never bakes them");
    if (count == 0) return GS_OK;
    ScopedDevice sd(s->ctx->device);
    GS_TRY(with_source_of(a, [&](auto source) { return sorter_upload_rows<typename decltype(source)::type>(s, from, a, first, count); }));
    return gs_sorter_commit_centers(s, from, count, scene_indexes);
}

}  // extern "C"
