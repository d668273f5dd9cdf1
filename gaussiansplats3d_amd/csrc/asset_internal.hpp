// asset_internal.hpp — what the host readers (assets.hip) and the device decode (asset_decode.hip) share: the parsed
// .ksplat image and the two half-float rules, each said once for both sides.
#pragma once
#include <math.h>

#include "gs_internal.hpp"

// THREE.DataUtils.toHalfFloat (three r160): clamp to +-65504, then the base/shift tables: the mantissa is TRUNCATED
__host__ __device__ inline uint16_t to_half_three(double value) {
    float v = (float)value;
    if (v > 65504.0f) v = 65504.0f;
    if (v < -65504.0f) v = -65504.0f;
    const uint32_t f = __builtin_bit_cast(uint32_t, v);
    const uint32_t sign = (f >> 16) & 0x8000u;
    const int e = (int)((f >> 23) & 0xFFu) - 127;
    const uint32_t m = f & 0x007FFFFFu;
    uint32_t out;
    if (e < -24) out = 0;
    else if (e < -14) out = (0x0400u >> (-e - 14)) + (m >> (-e - 1));
    else if (e <= 15) out = ((uint32_t)(e + 15) << 10) + (m >> 13);
    else if (e < 128) out = 0x7C00u;
    else out = 0x7C00u + (m >> 13);
    return (uint16_t)(out | sign);
}

__host__ __device__ inline double from_half(uint16_t h) {          // exact
    const uint32_t sign = h & 0x8000u, e = (h >> 10) & 31u, m = h & 1023u;
    double v;
    if (e == 0) v = ldexp((double)m, -24);
    else if (e == 31) v = m ? (double)NAN : (double)INFINITY;
    else v = ldexp((double)(m | 1024u), (int)e - 25);
    return sign ? -v : v;
}

struct AssetSection {
    uint32_t splat_count, max_splat_count, bucket_size, bucket_count, full_buckets, partial_buckets, sh_degree;
    uint32_t bytes_per_splat, scale_range;
    double half_block, scale_factor;
    size_t base, buckets_base, data_base;
    uint32_t count_offset;
    uint32_t bucket_storage;
    std::vector<uint32_t> partial_end;     // cumulative end (in section-local splats) of every partial bucket
};

constexpr uint32_t ASSET_CENTER_BYTES[3] = {12, 6, 6}, ASSET_SCALE_BYTES[3] = {12, 6, 6}, ASSET_ROT_BYTES[3] = {16, 8, 8},
                   ASSET_SH_BYTES_PER[3] = {4, 2, 1};
__host__ __device__ inline uint32_t asset_center_bytes(uint32_t level) { return level == 0 ? 12u : 6u; }     // = scale bytes
__host__ __device__ inline uint32_t asset_rotation_bytes(uint32_t level) { return level == 0 ? 16u : 8u; }
__host__ __device__ inline uint32_t sh_components(uint32_t degree) { return degree == 0 ? 0u : (degree == 1 ? 9u : 24u); }

struct gs_asset {
    std::vector<uint8_t> buf;              // a .ksplat image (for a PLY: the level-0 section built from it)
    uint32_t level = 0, splat_count = 0, sh_degree = 0;
    float scene_center[3] = {0, 0, 0};
    double sh_min = -1.5, sh_max = 1.5;
    std::vector<AssetSection> sections;
    std::vector<uint32_t> section_of;      // per splat

    template <class T>
    T rd(size_t off) const {
        T v;
        memcpy(&v, buf.data() + off, sizeof(T));
        return v;
    }
};
