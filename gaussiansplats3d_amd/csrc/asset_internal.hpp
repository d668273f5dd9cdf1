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

// Util.js clamp = Math.max(Math.min(v, hi), lo): JS min / max PROPAGATE NaN (C's fmin / fmax drop it)
__host__ __device__ inline double clampd(double v, double lo, double hi) {
    if (v != v) return v;
    return v > hi ? hi : (v < lo ? lo : v);
}

__host__ __device__ inline uint8_t to_uint8_range(double v, double lo, double hi) {   // SplatBuffer.js:22-26
    v = clampd(v, lo, hi);
    const double r = clampd(floor((v - lo) / (hi - lo) * 255.0), 0.0, 255.0);
    return r == r ? (uint8_t)r : (uint8_t)0;                                          // a NaN stored into a Uint8Array is 0
}

// ---- the static scene transform (gs_asset_set_transform) ---------------------------------------------------------------
// What SplatMesh.fillSplatDataArrays hands to the SplatBuffer fills in static mode, and what fillSphericalHarmonicsArray
// derives from it once per call (SplatBuffer.js:628-637, 781-815).  Travels by value in the kernel argument.
struct AssetTransform {
    double m[16];          // THREE.Matrix4.elements, column-major
    double sh1[3][3];      // sh11, sh12, sh13: the band-1 rows
    double sh2[5][5];      // sh21 .. sh25: the band-2 rows
};

// A typed-array store of a NaN keeps no particular bit pattern in the reference; the host and the device generate NaNs of
// different signs (0 * inf), so the transformed stores write the canonical quiet NaN on both sides.
__host__ __device__ inline float xf_f32(double v) { return v != v ? __builtin_bit_cast(float, 0x7FC00000u) : (float)v; }
__host__ __device__ inline uint16_t xf_f16(double v) { return v != v ? (uint16_t)0x7E00u : to_half_three(v); }

// Vector3.applyMatrix4 on the double centre (SplatBuffer.js:340-345), narrowed to float on store
__host__ __device__ inline void xf_centre(const AssetTransform& t, const double c[3], float out[3]) {
#pragma clang fp contract(off)
    const double x = c[0], y = c[1], z = c[2];
    const double* e = t.m;
    const double w = 1 / (e[3] * x + e[7] * y + e[11] * z + e[15]);
    out[0] = xf_f32((e[0] * x + e[4] * y + e[8] * z + e[12]) * w);
    out[1] = xf_f32((e[1] * x + e[5] * y + e[9] * z + e[13]) * w);
    out[2] = xf_f32((e[2] * x + e[6] * y + e[10] * z + e[14]) * w);
}

// computeCovariance's `if (transform)` (SplatBuffer.js:461-466): C.multiply(T3^T), then C.premultiply(T3), both
// Matrix3.multiplyMatrices' three-term sums.  T3 = Matrix3.setFromMatrix4(transform): T3[r][c] = m[r + 4c].
// out: elements 0,3,6,4,7,8 (the upper triangle; the product is not exactly symmetric)
__host__ __device__ inline void xf_covariance(const AssetTransform& t, const double C[3][3], double e[6]) {
#pragma clang fp contract(off)
    double A[3][3], B[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[r][c] = C[r][0] * t.m[c] + C[r][1] * t.m[c + 4] + C[r][2] * t.m[c + 8];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) B[r][c] = t.m[r] * A[0][c] + t.m[r + 4] * A[1][c] + t.m[r + 8] * A[2][c];
    e[0] = B[0][0]; e[1] = B[0][1]; e[2] = B[0][2]; e[3] = B[1][1]; e[4] = B[1][2]; e[5] = B[2][2];
}

// toUncompressedFloat(isSH = true) of a file value (SplatBuffer.js:12-31): level 0 fp32, 1 half, 2 v/255*(max-min)+min
__host__ __device__ inline double sh_widen(uint32_t level, const uint8_t* p, uint32_t index, double sh_min, double sh_max) {
#pragma clang fp contract(off)
    if (level == 0) { float v; __builtin_memcpy(&v, p + 4 * (size_t)index, 4); return (double)v; }
    if (level == 1) { uint16_t v; __builtin_memcpy(&v, p + 2 * (size_t)index, 2); return from_half(v); }
    return (double)p[index] / 255 * (sh_max - sh_min) + sh_min;
}

// fillSphericalHarmonicsArray with a transform (SplatBuffer.js:678-729): widen, rotateSphericalHarmonics3 / 5 (dot3 / dot5:
// the accumulator starts at 0, the terms are added in order), convert FROM LEVEL 0 to the output level.  hrow: the splat's SH
// in the file; out(dst, v) stores component dst of the splat.
template <class Out>
__host__ __device__ inline void xf_sh(const AssetTransform& t, uint32_t level, uint32_t degree, double sh_min, double sh_max,
                                      const uint8_t* hrow, Out out) {
#pragma clang fp contract(off)
    for (uint32_t ch = 0; ch < 3; ch++) {                                              // set3FromArray(stride 3, base c)
        double in[3];
        for (uint32_t q = 0; q < 3; q++) in[q] = sh_widen(level, hrow, q + 3 * ch, sh_min, sh_max);
        for (uint32_t j = 0; j < 3; j++) {
            double acc = 0.0;
            for (uint32_t q = 0; q < 3; q++) acc = acc + in[q] * t.sh1[j][q];
            out(3 * j + ch, acc);
        }
    }
    if (degree < 2) return;
    for (uint32_t ch = 0; ch < 3; ch++) {                                              // set3FromArray(stride 5, base 9 + c)
        double in[5];
        for (uint32_t q = 0; q < 5; q++) in[q] = sh_widen(level, hrow, 9 + q + 5 * ch, sh_min, sh_max);
        for (uint32_t j = 0; j < 5; j++) {
            double acc = 0.0;
            for (uint32_t q = 0; q < 5; q++) acc = acc + in[q] * t.sh2[j][q];
            out(9 + 3 * j + ch, acc);
        }
    }
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
    bool has_transform = false;            // gs_asset_set_transform
    AssetTransform xf = {};

    template <class T>
    T rd(size_t off) const {
        T v;
        memcpy(&v, buf.data() + off, sizeof(T));
        return v;
    }
};
