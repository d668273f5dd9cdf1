// asset_internal.hpp — what the host readers (assets.hip) and the device decode (asset_decode.hip) share, each said once as
// __host__ __device__ code for both sides: the two half-float rules, the scene transform, the per-row arithmetic of the formats
// whose file rows are decoded on both sides (.splat, PlayCanvas compressed PLY, .spz, INRIA-v2 codebook PLY, streamed INRIA-v1 PLY), the .ksplat row
// reader (KsplatSource) and the per-splat fill (asset_fill_splat) that gs_asset_fill loops over and k_asset_decode runs one thread of.
#pragma once
#include <math.h>

#include <memory>

#include "asset_stream.hpp"
#include "gs_internal.hpp"
#include "spz_container.hpp"

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
// the accumulator starts at 0, the terms are added in order), convert FROM LEVEL 0 to the output level.  wide(src): the
// widened value of the splat's SH with file index src; out(dst, v) stores component dst of the splat.  Inlined into its one
// caller, asset_fill_splat: out of line, the closures' captures would live in memory.
template <class In, class Out>
__host__ __device__ __forceinline__ void xf_sh(const AssetTransform& t, uint32_t degree, In wide, Out out) {
#pragma clang fp contract(off)
    for (uint32_t ch = 0; ch < 3; ch++) {                                              // set3FromArray(stride 3, base c)
        double in[3];
        for (uint32_t q = 0; q < 3; q++) in[q] = wide(q + 3 * ch);
        for (uint32_t j = 0; j < 3; j++) {
            double acc = 0.0;
            for (uint32_t q = 0; q < 3; q++) acc = acc + in[q] * t.sh1[j][q];
            out(3 * j + ch, acc);
        }
    }
    if (degree < 2) return;
    for (uint32_t ch = 0; ch < 3; ch++) {                                              // set3FromArray(stride 5, base 9 + c)
        double in[5];
        for (uint32_t q = 0; q < 5; q++) in[q] = wide(9 + q + 5 * ch);
        for (uint32_t j = 0; j < 5; j++) {
            double acc = 0.0;
            for (uint32_t q = 0; q < 5; q++) acc = acc + in[q] * t.sh2[j][q];
            out(9 + 3 * j + ch, acc);
        }
    }
}

// ---- file rows decoded on both sides: .splat and PlayCanvas compressed PLY ---------------------------------------------------
// file row (+ chunk row) -> the level-0 tuple the reference would store for it (SplatBuffer level 0: 3 centre floats, 3 scales,
// 4 rotation floats in file slot order, 4 colour bytes) and the SH floats.  The host image builder (assets.hip) and the row
// sources of the kernels (asset_decode.hip) both call these; every operation is IEEE-exact on both sides (+ - * / sqrt floor
// ceil and conversions, unfused), and exp is row_exp below, one implementation compiled for both.  Restates, never copies:
//   .splat row        src/loaders/splat/SplatParser.js:13-56
//   compressed row    src/loaders/ply/PlayCanvasCompressedPlyParser.js:21-65 (unpack*, lerp), :379-432 (decompressBaseSplat),
//                     :434-460 (decompressSphericalHarmonics) + SplatBuffer.writeSplatDataToSectionBuffer :1092-1124
struct Level0Tuple {
    float c[3], s[3], r[4];    // r: the level-0 row's four rotation floats in slot order (slot 0 is read back as w)
    uint8_t rgba[4];
};

// A NaN this decode GENERATES (lerp over infinite extremes, sqrt of a negative) has one sign on the host and the other on the
// device; a typed-array store keeps no particular NaN either.  Stored as the canonical quiet NaN on both sides (xf_f32's rule).
__host__ __device__ inline float row_f32(double v) { return xf_f32(v); }

// e^x in double for the compressed PLY's scales.  The argument reduction and the degree-5 remainder polynomial of the freely
// distributable fdlibm e_exp (Sun Microsystems, 1993; the algorithm JavaScript engines ship as Math.exp), restated with
// + - * / only, so the host and the device compute the same bits - libm here and the device library there would agree to 1 ulp
// and then disagree after narrowing to fp32 about once in 2^29 values.
__host__ __device__ inline double row_exp(double x) {
#pragma clang fp contract(off)
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    const uint32_t hx = (uint32_t)(bits >> 32) & 0x7FFFFFFFu;
    const int neg = (int)(bits >> 63);
    if (hx >= 0x40862E42u) {                                               // |x| >= 709.78: NaN, inf, overflow, underflow
        if (hx >= 0x7FF00000u) {
            if ((bits & 0x000FFFFFFFFFFFFFull) != 0) return x + x;        // NaN
            return neg ? 0.0 : x;
        }
        if (x > 7.09782712893383973096e+02) return __builtin_bit_cast(double, 0x7FF0000000000000ull);
        if (x < -7.45133219101941108420e+02) return 0.0;
    }
    double hi = 0.0, lo = 0.0;
    int k = 0;
    if (hx > 0x3FD62E42u) {                                                // |x| > 0.5 ln2
        if (hx < 0x3FF0A2B2u) {                                            // and < 1.5 ln2
            hi = neg ? x + ln2_hi : x - ln2_hi;
            lo = neg ? -ln2_lo : ln2_lo;
            k = neg ? -1 : 1;
        } else {
            k = (int)(inv_ln2 * x + (neg ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2_hi;
            lo = t * ln2_lo;
        }
        x = hi - lo;
    } else if (hx < 0x3E300000u) {                                         // |x| < 2^-28
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k >= -1021) {
        if (k == 1024) return y * 2.0 * __builtin_bit_cast(double, 0x7FE0000000000000ull);
        return y * __builtin_bit_cast(double, (uint64_t)(0x3FF + k) << 52);
    }
    return y * __builtin_bit_cast(double, (uint64_t)(0x3FF + k + 1000) << 52) * __builtin_bit_cast(double, 0x0170000000000000ull);   // 2^-1000
}

// Quaternion.normalize (three r160) on q = x, y, z, w
__host__ __device__ inline void row_normalize(double q[4]) {
#pragma clang fp contract(off)
    double l = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (l == 0) { q[0] = q[1] = q[2] = 0; q[3] = 1; }
    else { l = 1 / l; for (int k = 0; k < 4; k++) q[k] = q[k] * l; }
}

// .splat: the row's eight dwords (centre 3 x f32, scale 3 x f32, RGBA, rotation bytes).  Scales and colours are copied;
// the quaternion is normalised once and stored w, x, y, z (SplatParser.js:28-49)
__host__ __device__ inline void splat_row_tuple(const uint32_t w[8], Level0Tuple& t) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) t.c[k] = __builtin_bit_cast(float, w[k]);
    for (int k = 0; k < 3; k++) t.s[k] = __builtin_bit_cast(float, w[3 + k]);
    for (int k = 0; k < 4; k++) t.rgba[k] = (uint8_t)(w[6] >> (8 * k));
    const double b0 = (double)(w[7] & 255u), b1 = (double)((w[7] >> 8) & 255u), b2 = (double)((w[7] >> 16) & 255u), b3 = (double)(w[7] >> 24);
    double q[4] = {(b1 - 128) / 128, (b2 - 128) / 128, (b3 - 128) / 128, (b0 - 128) / 128};
    row_normalize(q);
    t.r[0] = (float)q[3]; t.r[1] = (float)q[0]; t.r[2] = (float)q[1]; t.r[3] = (float)q[2];
}

// PlayCanvas compressed PLY: where a splat's values lie in its 16-byte vertex row and its chunk row, from the header
enum { PC_MIN_POS = 0, PC_MAX_POS = 3, PC_MIN_SCALE = 6, PC_MAX_SCALE = 9, PC_MIN_COL = 12, PC_MAX_COL = 15 };
struct PcLayout {
    int32_t ext[18];           // byte offset in a chunk row of min_x/y/z, max_x/y/z, min_scale_x/y/z, max_scale_x/y/z, min_r/g/b,
                               // max_r/g/b (float); the colour ones are -1 when the chunk element has none
    uint32_t word[4];          // dword of packed_position, packed_rotation, packed_scale, packed_color in a vertex row
    uint32_t chunk_stride;     // bytes per chunk row
    uint32_t chunk_aligned;    // stride and every offset are multiples of 4: a chunk float is one aligned load
    uint32_t sh_stride;        // SH properties (bytes) per splat: 9 / 24 / 45 for a well-formed file
    uint32_t read_coeff;       // readSHCoeff 3 / 8 / 15: the stride of shArray[j * readSHCoeff + k]
};

__host__ __device__ inline double pc_chunk_f32(const uint8_t* chunk, const PcLayout& L, int which) {
    float v;
    const uint8_t* p = chunk + L.ext[which];
#if defined(__HIP_DEVICE_COMPILE__)
    if (L.chunk_aligned) return (double)*reinterpret_cast<const float*>(p);   // the staged chunk rows start 16-byte aligned
#endif
    __builtin_memcpy(&v, p, 4);
    return (double)v;
}
__host__ __device__ inline double pc_unorm(uint32_t value, uint32_t bits) {           // unpackUnorm: divides in double
    const uint32_t t = (1u << bits) - 1u;
    return (double)(value & t) / (double)t;
}
__host__ __device__ inline double pc_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    return a * (1 - t) + b * t;
}
__host__ __device__ inline void pc_unpack111011(uint32_t v, double out[3]) {
    out[0] = pc_unorm(v >> 21, 11); out[1] = pc_unorm(v >> 11, 10); out[2] = pc_unorm(v, 11);
}

// the centre alone (what the sorter's message needs): the position word and the chunk's six position extremes
__host__ __device__ inline void pc_row_centre(uint32_t position, const uint8_t* chunk, const PcLayout& L, float c[3]) {
    double p[3];
    pc_unpack111011(position, p);
    for (int k = 0; k < 3; k++) c[k] = row_f32(pc_lerp(pc_chunk_f32(chunk, L, PC_MIN_POS + k), pc_chunk_f32(chunk, L, PC_MAX_POS + k), p[k]));
}

// JS Math.round: the nearest integer, ties towards +inf
__host__ __device__ inline double js_round(double v) {
    const double r = ceil(v);
    return r - 0.5 > v ? r - 1.0 : r;
}

// decompressBaseSplat, then the level-0 store of writeSplatDataToSectionBuffer: normalise, `|| 0` on the scales and colours
__host__ __device__ inline void pc_row_tuple(const uint32_t w[4], const uint8_t* chunk, const PcLayout& L, Level0Tuple& t) {
#pragma clang fp contract(off)
    pc_row_centre(w[L.word[0]], chunk, L, t.c);
    {   // unpackRot: 2 + 10 + 10 + 10, the largest component dropped and rebuilt
        const uint32_t v = w[L.word[1]];
        const double norm = 1.0 / (1.4142135623730951 * 0.5);                          // 1.0 / (Math.sqrt(2) * 0.5)
        const double a = (pc_unorm(v >> 20, 10) - 0.5) * norm, b = (pc_unorm(v >> 10, 10) - 0.5) * norm, c = (pc_unorm(v, 10) - 0.5) * norm;
        const double m = sqrt(1.0 - (a * a + b * b + c * c));
        double q[4];                                                                   // Quaternion.set(x, y, z, w)
        switch (v >> 30) {
            case 0: q[0] = m; q[1] = a; q[2] = b; q[3] = c; break;
            case 1: q[0] = a; q[1] = m; q[2] = b; q[3] = c; break;
            case 2: q[0] = a; q[1] = b; q[2] = m; q[3] = c; break;
            default: q[0] = a; q[1] = b; q[2] = c; q[3] = m; break;
        }
        row_normalize(q);                                                              // tempRot.normalize() :1093-1094
        for (int k = 0; k < 4; k++) t.r[k] = row_f32(q[k]);                            // rot.set([x, y, z, w]) :1112
    }
    {
        double s[3];
        pc_unpack111011(w[L.word[2]], s);
        for (int k = 0; k < 3; k++) {
            const double e = row_exp(pc_lerp(pc_chunk_f32(chunk, L, PC_MIN_SCALE + k), pc_chunk_f32(chunk, L, PC_MAX_SCALE + k), s[k]));
            t.s[k] = (float)(e == e ? e : 0.0);                                        // `|| 0`
        }
    }
    {   // unpack8888
        const uint32_t v = w[L.word[3]];
        for (int k = 0; k < 3; k++) {
            const double c = pc_unorm(v >> (24 - 8 * k), 8);
            double o;
            if (L.ext[PC_MIN_COL + k] >= 0 && L.ext[PC_MAX_COL + k] >= 0)
                o = clampd(js_round(pc_lerp(pc_chunk_f32(chunk, L, PC_MIN_COL + k), pc_chunk_f32(chunk, L, PC_MAX_COL + k), c) * 255), 0, 255);
            else
                o = clampd(floor(c * 255), 0, 255);
            t.rgba[k] = o == o ? (uint8_t)o : (uint8_t)0;                              // `|| 0`; an integer in 0..255 otherwise
        }
        t.rgba[3] = (uint8_t)clampd(floor(pc_unorm(v, 8) * 255), 0, 255);
    }
}

// SH float s (0..8 band 1, 9..23 band 2, the level-0 row's order) of a splat whose SH bytes start at sh: the inverse of the
// reference's shIndexMap over shArray[j * readSHCoeff + k], value * (8 / 255) - 4, stored fp32
__host__ __device__ inline float pc_row_sh(const uint8_t* sh, uint32_t read_coeff, uint32_t s) {
#pragma clang fp contract(off)
    const uint32_t j = s < 9u ? s / 3u : (s - 9u) / 5u, k = s < 9u ? s % 3u : 3u + (s - 9u) % 5u;
    return (float)((double)sh[j * read_coeff + k] * (8.0 / 255.0) - 4);
}

// ---- .spz: six byte planes -> the level-0 tuple --------------------------------------------------------------------------------
// Restates, never copies: src/loaders/spz/SpzLoader.js:160-250 (unpackGaussians), :84-145 (unpackedSplatToUncompressedSplat), then
// the level-0 store of SplatBuffer.writeSplatDataToSectionBuffer :1092-1124, 1168-1172.  A splat's bytes as both sides hand them over:
struct SpzRowBytes {
    uint32_t pos[3];           // version 2: three bytes little endian in bits 0..23; version 1: half bits
    uint32_t alpha;            // the byte
    uint32_t colour, scale, rotation;   // three bytes each, byte k in bits 8k .. 8k + 7
};

// the centre: 24-bit fixed point, sign-extended from bit 23, times the position scale (SpzLoader.js:196-204), or a half (:190-194:
// halfToFloat is exact, as from_half is, for -0, inf and NaN too); stored fp32 (SplatBuffer.js:1114)
__host__ __device__ inline void spz_row_centre(const SpzLayout& L, const uint32_t pos[3], float c[3]) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) {
        if (L.pos_stride == 9u) c[k] = (float)((double)((int32_t)(pos[k] << 8) >> 8) * L.pos_scale);
        else c[k] = row_f32(from_half((uint16_t)pos[k]));
    }
}

__host__ __device__ inline void spz_row_tuple(const SpzLayout& L, const SpzRowBytes& b, Level0Tuple& t) {
#pragma clang fp contract(off)
    spz_row_centre(L, b.pos, t.c);
    for (int k = 0; k < 3; k++) t.s[k] = (float)row_exp((double)((b.scale >> (8 * k)) & 255u) / 16.0 - 10.0);   // :209; never 0 or NaN
    {
        const double x = (double)(b.rotation & 255u) / 127.5 - 1.0, y = (double)((b.rotation >> 8) & 255u) / 127.5 - 1.0,
                     z = (double)((b.rotation >> 16) & 255u) / 127.5 - 1.0;
        const double rest = 1.0 - (x * x + y * y + z * z);
        // Quaternion.set(x = w, y = x, z = y, w = z) :132: row_normalize sums the squares in exactly that slot order.  Normalised
        // there (:133) and AGAIN by writeSplatDataToSectionBuffer (SplatBuffer.js:1093-1094); one pass is not bit-equal to two.
        double q[4] = {sqrt(rest > 0.0 ? rest : 0.0), x, y, z};
        row_normalize(q);
        row_normalize(q);
        for (int k = 0; k < 4; k++) t.r[k] = (float)q[k];
    }
    for (int k = 0; k < 3; k++) {                                                      // :231, then clamp(floor(.)) :116-118
        const double c = (double)((b.colour >> (8 * k)) & 255u);
        t.rgba[k] = (uint8_t)clampd(floor(floor((((c / 255.0 - 0.5) / 0.15) * 0.28209479177387814 + 0.5) * 255)), 0, 255);
    }
    t.rgba[3] = (uint8_t)b.alpha;                                                      // min_alpha zeroes it at fill time only
}

// Level-0 SH slot s (0..8 band 1, 9..23 band 2) -> the byte's index within the splat's 3 * dim SH bytes: coefficient k of channel j
// lies at 3 * k + j (:237), and slot s holds j = s / 3, k = s % 3 below 9, j = (s - 9) / 5, k = 3 + (s - 9) % 5 above (the inverse of
// the reference's shIndexMap, as pc_row_sh states it).  The caller only asks for slots of a degree min(output, file) <= 2: k < dim.
__host__ __device__ inline uint32_t spz_sh_index(uint32_t s) {
    const uint32_t j = s < 9u ? s / 3u : (s - 9u) / 5u, k = s < 9u ? s % 3u : 3u + (s - 9u) % 5u;
    return 3u * k + j;
}
__host__ __device__ inline float spz_sh_value(uint32_t byte) {                         // unquantizeSH :31-33, stored fp32
#pragma clang fp contract(off)
    return (float)(((double)byte - 128.0) / 128.0);
}

// ---- INRIA-v2 codebook PLY: one index byte per attribute -> the level-0 tuple ---------------------------------------------------------
// Restates, never copies: src/loaders/ply/INRIAV2PlyParser.js:202-269 (parseToUncompressedSplat), then the level-0 store of
// SplatBuffer.writeSplatDataToSectionBuffer :1092-1124, 1168-1172.  The codebook is decoded ONCE, at open, on the host (assets.hip:
// decodeCodeBook :128-160 and every per-row rule that depends on the entry alone), so all a row needs of an entry is one fp32 and
// a row's decode is look-ups, the three centre halves and the quaternion's two normalisations.  The decoded table's pages, 256
// floats each, in the order the output degrees read them: a degree reads the first inria_v2_pages_read(degree) pages.
enum { IV2_PAGE_DC = 0, IV2_PAGE_OPACITY = 1, IV2_PAGE_SCALING = 2, IV2_PAGE_ROTATION_RE = 3, IV2_PAGE_ROTATION_IM = 4,
       IV2_PAGE_REST = 5, IV2_PAGES = 20, IV2_ABSENT = 0xFFFF };
__host__ __device__ inline uint32_t inria_v2_pages_read(uint32_t degree) { return IV2_PAGE_REST + (degree == 0 ? 0u : (degree == 1 ? 3u : 8u)); }

// Where a splat's values lie in its file row, from the header (every offset < stride < 64 KiB).  x / y / z and rot_0..3 always
// exist; any other field may be IV2_ABSENT, which reads as the reference reads `undefined`.
struct InriaV2Layout {
    uint32_t stride;           // bytes per file row
    uint16_t pos[3];           // x, y, z: half bits
    uint16_t rot[4], scale[3], dc[3], opacity;   // index bytes
    uint16_t sh[24];           // the index byte of level-0 SH slot s: f_rest_{s%3 + cpc*(s/3)} below 9, f_rest_{3 + (s-9)%5 + cpc*((s-9)/5)} above
};

__host__ __device__ inline float inria_v2_entry(const float* codebook, uint32_t page, uint32_t index) { return codebook[256u * page + index]; }

// the centre alone: fromHalfFloat of the three 16-bit words (:264-266; exact, as from_half is), stored fp32
__host__ __device__ inline void inria_v2_row_centre(const uint8_t* row, const InriaV2Layout& L, float c[3]) {
    for (int k = 0; k < 3; k++) c[k] = row_f32(from_half((uint16_t)((uint32_t)row[L.pos[k]] | ((uint32_t)row[L.pos[k] + 1u] << 8))));
}

__host__ __device__ inline void inria_v2_row_tuple(const uint8_t* row, const InriaV2Layout& L, const float* codebook, Level0Tuple& t) {
#pragma clang fp contract(off)
    inria_v2_row_centre(row, L, t.c);
    for (int k = 0; k < 3; k++) {                                                      // :206-214; a missing scale_1 / 2 is `undefined || 0`
        if (L.scale[0] == IV2_ABSENT) t.s[k] = (float)0.01;
        else t.s[k] = L.scale[k] == IV2_ABSENT ? 0.0f : inria_v2_entry(codebook, IV2_PAGE_SCALING, row[L.scale[k]]);
    }
    {   // :252-262 Quaternion.set(rot_0..3).normalize(), then the second normalize of writeSplatDataToSectionBuffer :1093-1094
        double q[4] = {(double)inria_v2_entry(codebook, IV2_PAGE_ROTATION_RE, row[L.rot[0]]), 0, 0, 0};
        for (int k = 1; k < 4; k++) q[k] = (double)inria_v2_entry(codebook, IV2_PAGE_ROTATION_IM, row[L.rot[k]]);
        row_normalize(q);
        row_normalize(q);
        for (int k = 0; k < 4; k++) t.r[k] = row_f32(q[k]);                            // an infinite entry: inf * (1 / inf) = a generated NaN
    }
    for (int k = 0; k < 3; k++)                                                        // :216-236; the red / green / blue branch is dead code
        t.rgba[k] = L.dc[0] == IV2_ABSENT || L.dc[k] == IV2_ABSENT ? (uint8_t)0 : (uint8_t)inria_v2_entry(codebook, IV2_PAGE_DC, row[L.dc[k]]);
    t.rgba[3] = L.opacity == IV2_ABSENT ? (uint8_t)0 : (uint8_t)inria_v2_entry(codebook, IV2_PAGE_OPACITY, row[L.opacity]);
}

// Level-0 SH float s of the row (:239-249): the pages are indexed by coefficient and shared by the three channels
__host__ __device__ inline float inria_v2_row_sh(const uint8_t* row, const InriaV2Layout& L, const float* codebook, uint32_t s) {
    if (L.sh[s] == IV2_ABSENT) return 0.0f;
    return inria_v2_entry(codebook, IV2_PAGE_REST + (s < 9u ? s % 3u : 3u + (s - 9u) % 5u), row[L.sh[s]]);
}

// ---- INRIA-v1 PLY: the trainer's own rows -> the level-0 tuple --------------------------------------------------------------------------
// Restates, never copies: src/loaders/ply/INRIAV1PlyParser.js:114-209 (parseToUncompressedSplat) + PlyParserUtils.readVertex, then the
// level-0 store of SplatBuffer.writeSplatDataToSectionBuffer :1056-1113 - the rules parse_ply (assets.hip) applies to a whole file, with
// row_exp where that calls libm's exp (one implementation for both sides; after the fp32 store and floor(. * 255) the two agree except
// on rare boundary inputs).  Only streamed assets read their rows through this (gs_asset_open_stream).
// Where the fields parse_ply maps lie in a file row, from the header: the row stride (< 64 KiB) and per field a present bit, a type
// and an offset.  A `double` property is never read by the reference (PlyParserUtils.js:281-301): it counts as absent.
enum : uint8_t { IV1_FLOAT = 0, IV1_INT = 1, IV1_UINT = 2, IV1_SHORT = 3, IV1_USHORT = 4, IV1_UCHAR = 5 };
struct InriaV1Field { uint16_t offset; uint8_t type, present; };
struct InriaV1Layout {
    uint32_t stride;           // bytes per file row: 68 at degree 0, 248 at degree 3, odd with a uchar property
    uint32_t aligned;          // the stride and the offset of every present 4-byte field are multiples of 4: with row 0 on a 16-byte
                               // boundary (the staging base) such a field is one aligned dword load on the device
    InriaV1Field pos[3], scale[3], rot[4], dc[3], rgb[3], opacity, rest0;
    InriaV1Field sh[24];       // level-0 SH slot s: f_rest_{s%3 + cpc*(s/3)} below 9, f_rest_{3 + (s-9)%5 + cpc*((s-9)/5)} above
};

// PlyParserUtils.readVertex for one field: false = `undefined`.  Nothing is known of a row's alignment on the host (the header has
// any length), and on the device only what `aligned` proves: everything else is put together from byte loads.
__host__ __device__ __forceinline__ bool inria_v1_read(const uint8_t* row, const InriaV1Layout& L, const InriaV1Field f, double* out) {
    if (!f.present) return false;
    const uint8_t* p = row + f.offset;
    if (f.type == IV1_UCHAR) { *out = (double)p[0] / 255.0; return true; }                // normalize = true
    if (f.type >= IV1_SHORT) {
        const uint32_t h = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
        *out = f.type == IV1_SHORT ? (double)(int16_t)h : (double)h;
        return true;
    }
    uint32_t w;
#if defined(__HIP_DEVICE_COMPILE__)
    if (L.aligned) w = *reinterpret_cast<const uint32_t*>(p);
    else
#endif
        w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    (void)L;
    *out = f.type == IV1_FLOAT ? (double)__builtin_bit_cast(float, w) : (f.type == IV1_INT ? (double)(int32_t)w : (double)w);
    return true;
}

// the centre alone: x, y, z as stored fp32 (an absent one is NaN)
__host__ __device__ inline void inria_v1_row_centre(const uint8_t* row, const InriaV1Layout& L, float c[3]) {
    for (int k = 0; k < 3; k++) {
        double v = (double)NAN;
        inria_v1_read(row, L, L.pos[k], &v);
        c[k] = (float)v;
    }
}

__host__ __device__ inline void inria_v1_row_tuple(const uint8_t* row, const InriaV1Layout& L, Level0Tuple& t) {
#pragma clang fp contract(off)
    double v, s3[3], r4[4] = {(double)NAN, (double)NAN, (double)NAN, (double)NAN}, col[3], op = 0.0;   // createSplat() starts every field at 0
    if (inria_v1_read(row, L, L.scale[0], &v)) {                                       // INRIAV1PlyParser.js:148-156
        for (int k = 0; k < 3; k++) { s3[k] = (double)NAN; if (inria_v1_read(row, L, L.scale[k], &v)) s3[k] = row_exp(v); }
    } else {
        s3[0] = s3[1] = s3[2] = 0.01;
    }
    if (inria_v1_read(row, L, L.dc[0], &v)) {                                          // :158-172
        const double SH_C0 = 0.28209479177387814;
        for (int k = 0; k < 3; k++) { col[k] = (double)NAN; if (inria_v1_read(row, L, L.dc[k], &v)) col[k] = (0.5 + SH_C0 * v) * 255; }
    } else if (inria_v1_read(row, L, L.rgb[0], &v)) {
        for (int k = 0; k < 3; k++) { col[k] = (double)NAN; if (inria_v1_read(row, L, L.rgb[k], &v)) col[k] = v * 255; }
    } else {
        col[0] = col[1] = col[2] = 0;
    }
    if (inria_v1_read(row, L, L.opacity, &v)) op = (1 / (1 + row_exp(-v))) * 255;       // :174-176
    for (int k = 0; k < 3; k++) col[k] = clampd(floor(col[k]), 0, 255);                // :178-181
    op = clampd(floor(op), 0, 255);
    // :196-202 Quaternion.set(rot_0..3).normalize(), then the second normalize of writeSplatDataToSectionBuffer :1084-1086
    for (int k = 0; k < 4; k++) if (inria_v1_read(row, L, L.rot[k], &v)) r4[k] = v;
    row_normalize(r4);
    row_normalize(r4);
    inria_v1_row_centre(row, L, t.c);
    for (int k = 0; k < 3; k++) t.s[k] = (float)(s3[k] == s3[k] ? s3[k] : 0.0);        // `|| 0`
    for (int k = 0; k < 4; k++) t.r[k] = row_f32(r4[k]);                               // an infinite component: inf * (1 / inf) = a generated NaN
    for (int k = 0; k < 3; k++) t.rgba[k] = col[k] == col[k] ? (uint8_t)col[k] : (uint8_t)0;   // Uint8ClampedArray store of an integer in 0..255, NaN -> 0
    t.rgba[3] = op == op ? (uint8_t)op : (uint8_t)0;
}

// Level-0 SH float s of the row (:183-194): read only when the row has an f_rest_0 (inria_v1_row_has_sh: asked once per row); an
// absent field is 0
__host__ __device__ inline bool inria_v1_row_has_sh(const uint8_t* row, const InriaV1Layout& L) {
    double v;
    return inria_v1_read(row, L, L.rest0, &v);
}
__host__ __device__ inline float inria_v1_row_sh(const uint8_t* row, const InriaV1Layout& L, bool has_sh, uint32_t s) {
    double v, c = 0;
    if (has_sh && inria_v1_read(row, L, L.sh[s], &v)) c = v;
    return (float)c;
}

// ---- .ksplat rows: one reader for the host fill and the kernels ------------------------------------------------------------------
// Restates, never copies: SplatBuffer.js:108-163 (rows per compression level), :199-219 (bucket of a splat), :221-246 (centre).
// Bytes of a row's parts per compression level, in row order: centre, scale, rotation, RGBA (4), SH
__host__ __device__ inline uint32_t asset_center_bytes(uint32_t level) { return level == 0 ? 12u : 6u; }
__host__ __device__ inline uint32_t asset_scale_bytes(uint32_t level) { return level == 0 ? 12u : 6u; }
__host__ __device__ inline uint32_t asset_rotation_bytes(uint32_t level) { return level == 0 ? 16u : 8u; }
__host__ __device__ inline uint32_t asset_sh_value_bytes(uint32_t level) { return level == 0 ? 4u : (level == 1 ? 2u : 1u); }
__host__ __device__ inline uint32_t sh_components(uint32_t degree) { return degree == 0 ? 0u : (degree == 1 ? 9u : 24u); }

// What a row read needs of one section.  parse_ksplat (assets.hip) fills it with offsets into the file image and proves every
// read through it in range; asset_stage (asset_decode.hip) copies the records of a range and rebases the offsets.
struct KsplatSection {
    long long data_off;        // byte offset of the section's row 0 in the image (negative in a staged range that starts inside the
                               // section: rows before the range are not uploaded)
    long long buckets_off;     // ... of its bucket centres
    uint32_t count_offset, count;            // its first splat, its splats (maxSplatCount: secLoadedCountsToMax)
    uint32_t bytes_per_splat, bucket_size, full_buckets, bucket_count, bucket_storage, scale_range;
    uint32_t partial_begin, partial_count;   // its slice of the image's cumulative partial_end list
    double scale_factor;
};

struct KsplatView {            // an image: the host's file, or what a kernel argument says of the staged range
    const uint8_t* image;
    const KsplatSection* sections;           // the non-empty sections in order
    const uint32_t* partial_end;             // cumulative end (in section-local splats) of every partial bucket
    uint32_t section_count, level, sh_degree, ncomp;
};

template <class T>
__host__ __device__ __forceinline__ T ld(const uint8_t* p) {   // rows have no alignment (33 bytes per splat at level 2, SH 1)
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// dataViewFloatForCompressionLevel for scale / rotation (never the 8-bit SH rule: that is sh_widen)
__host__ __device__ __forceinline__ double comp(uint32_t level, const uint8_t* row, uint32_t index) {
    if (level == 0) return (double)ld<float>(row + 4 * index);
    return from_half(ld<uint16_t>(row + 2 * index));
}

// the section of splat i: the last one that begins at or before it
__host__ __device__ __forceinline__ const KsplatSection& section_of(const KsplatView& v, uint32_t i) {
    uint32_t lo = 0, hi = v.section_count;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.sections[mid].count_offset <= i) lo = mid;
        else hi = mid;
    }
    return v.sections[lo];
}

// SplatBuffer.js:199-219: full buckets first, then the partial ones by their stored lengths.  parse_ksplat proved that the
// tables cover every splat, so the result is always < bucket_count; the clamp is never taken.
__host__ __device__ __forceinline__ uint32_t bucket_index(const KsplatView& v, const KsplatSection& sec, uint32_t local) {
    const uint32_t full_span = sec.full_buckets * sec.bucket_size;
    if (local < full_span) return local / sec.bucket_size;
    const uint32_t* pe = v.partial_end + sec.partial_begin;
    uint32_t lo = 0, hi = sec.partial_count;                    // first partial bucket whose end is > local
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pe[mid] <= local) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t b = sec.full_buckets + lo;
    return b < sec.bucket_count ? b : sec.bucket_count - 1u;    // never past the table
}

// getSplatCenter (SplatBuffer.js:221-246) in double
__host__ __device__ __forceinline__ void ksplat_centre(const KsplatView& v, const KsplatSection& sec, uint32_t local, const uint8_t* row,
                                                       double d[3]) {
    if (v.level == 0) {
        for (int k = 0; k < 3; k++) d[k] = ld<float>(row + 4 * k);
    } else {
        const uint8_t* bucket = v.image + sec.buckets_off + (size_t)sec.bucket_storage * bucket_index(v, sec, local);
        for (int k = 0; k < 3; k++) {
            const double x = ld<uint16_t>(row + 2 * k);
            const double bc = ld<float>(bucket + 4 * k);
            d[k] = (x - (double)sec.scale_range) * sec.scale_factor + bc;
        }
    }
}

// ---- row sources -----------------------------------------------------------------------------------------------------------------
// A source says where splat i's values come from.  Its Row gives: the double centre, the doubles of scale and rotation
// (w, x, y, z) as the fills read them, the colour bytes, and the SH of file index `src` in each of the three forms the store needs
// (widened double for the rotated fill, half bits, the level-2 byte).  This one reads a .ksplat image on either side; the
// kernels' sources over file rows of the other formats are in asset_decode.hip.
struct KsplatSource : KsplatView {
    struct Row {
        const KsplatView& v;
        const KsplatSection& sec;
        uint32_t local;
        const uint8_t* row;
        __host__ __device__ __forceinline__ const uint8_t* srow() const { return row + asset_center_bytes(v.level); }
        __host__ __device__ __forceinline__ const uint8_t* crow() const { return srow() + asset_scale_bytes(v.level) + asset_rotation_bytes(v.level); }
        __host__ __device__ __forceinline__ void centre(double d[3]) const { ksplat_centre(v, sec, local, row, d); }
        __host__ __device__ __forceinline__ void scale_rotation(double s[3], double q[4]) const {
            for (int k = 0; k < 3; k++) s[k] = comp(v.level, srow(), k);
            for (int k = 0; k < 4; k++) q[k] = comp(v.level, srow(), 3 + k);
        }
        __host__ __device__ __forceinline__ uint32_t colour() const { return ld<uint32_t>(crow()); }
        __host__ __device__ __forceinline__ double sh_wide(uint32_t src, double lo, double hi) const { return sh_widen(v.level, crow() + 4, src, lo, hi); }
        __host__ __device__ __forceinline__ uint16_t sh_half(uint32_t src) const {      // level 0 through the half rule, level 1 bits
            return v.level == 0 ? to_half_three((double)ld<float>(crow() + 4 + 4 * src)) : ld<uint16_t>(crow() + 4 + 2 * src);
        }
        __host__ __device__ __forceinline__ uint8_t sh_byte(uint32_t src) const { return crow()[4 + src]; }
    };
    __host__ __device__ __forceinline__ Row row(uint32_t splat) const {
        const KsplatSection& sec = section_of(*this, splat);
        const uint32_t local = splat - sec.count_offset;
        return Row{*this, sec, local, image + sec.data_off + (long long)sec.bytes_per_splat * local};
    }
    __host__ __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const { row(splat).centre(d); }
};

// ---- the per-splat fill: gs_asset_fill's loop body and k_asset_decode's thread -----------------------------------------------------
// Restates, never copies: covariance SplatBuffer.js:440-486, 517-549 (three.js Matrix3/4 arithmetic in double); colour :551-575;
// SH order :577-734; with a transform :340-342, 461-466, 684-688, 707-715, 736-770.  fp64 and unfused on both sides (the
// pragma here, -ffp-contract=off on both translation units): only multiplies, adds and double -> float conversions, so what
// gs_mesh_upload_asset leaves is bit-equal to gs_asset_fill + gs_mesh_upload (+ gs_mesh_upload_sh_u8).
// the double centre through the scene transform (SplatBuffer.js:332-342) or narrowed to float as fillSplatCenterArray stores it
template <bool XF>
__host__ __device__ __forceinline__ void store_centre(const AssetTransform& t, const double d[3], float c[3]) {
    if constexpr (XF) xf_centre(t, d, c);
    else for (int k = 0; k < 3; k++) c[k] = (float)d[k];
}

// splat `row` -> element i of the outputs.  XF: with the transform t (never read otherwise); sh_lo / sh_hi: the file's 8-bit SH range
// (read with XF only); ncomp = sh_components(sh_degree) of the OUTPUT degree.
// A kernel (HOST false) writes every plane of the staging layout (MeshStaging), one covariance width and one SH form: whichever
// pointer of each pair is set; scales / rotations are never looked at.  The host fill (HOST true) may leave any output out, may
// ask for both covariance widths, and has scales / rotations on top.  HOST settles that at compile time: the kernels carry none
// of the host's checks.  Rgba: uint32_t on the device (one aligned word), uint8_t on the host (the C ABI asks for no alignment).
// SURFEL (kernels only, never with XF): the mesh is a GS_MESH_SURFEL one and cov_f32 receives, in place of the covariance, the tuple
// (sx, sy, 1, qx, qy, qz) - the host's `scales` and `rotations` outputs with the scaleOverride.z = 1 of SplatMesh.fillSplatDataArrays
// in 2D mode (SplatMesh.js:1856-1863), as SplatMesh.updateScaleRotationsPaddedData stores them (:1155-1170).
template <bool XF, bool HOST, bool SURFEL = false, class Row, class Rgba>
__host__ __device__ __forceinline__ void asset_fill_splat(const Row row, const AssetTransform& t, uint32_t sh_degree, uint32_t ncomp,
                                                          double sh_lo, double sh_hi, uint32_t min_alpha, uint32_t i, float* centers,
                                                          float* cov_f32, uint16_t* cov_f16, Rgba* rgba, uint16_t* sh_f16, uint8_t* sh_u8,
                                                          float* scales, float* rotations) {
#pragma clang fp contract(off)
    if (!HOST || centers) {
        double d[3];
        float c[3];
        row.centre(d);
        store_centre<XF>(t, d, c);
        for (int k = 0; k < 3; k++) centers[3 * (size_t)i + k] = c[k];
    }
    if (!HOST || cov_f32 || cov_f16 || scales || rotations) {
        double s3[3], q4[4];
        row.scale_rotation(s3, q4);
        const double sx = s3[0], sy = s3[1], sz = s3[2];
        // rotation.set(x = f4, y = f5, z = f6, w = f3): NOT normalised (SplatBuffer.js:539-542)
        const double w = q4[0], x = q4[1], y = q4[2], z = q4[3];
        if constexpr (HOST) {
            if (scales) for (int k = 0; k < 3; k++) scales[3 * (size_t)i + k] = (float)s3[k];
            if (rotations) {   // fillSplatScaleRotationArray (SplatBuffer.js:407-424): Quaternion.normalize, then ensurePositiveW
                double q[4] = {x, y, z, w};
                row_normalize(q);
                const double flip = q[3] < 0 ? -1 : 1;
                for (int k = 0; k < 4; k++) rotations[4 * (size_t)i + k] = (float)(q[k] * flip);
            }
        }
        if constexpr (SURFEL) {
            static_assert(!HOST && !XF, "the surfel tuple is a device output of the untransformed fill");
            double q[4] = {x, y, z, w};                // as `rotations` above: Quaternion.normalize, then ensurePositiveW
            row_normalize(q);
            const double flip = q[3] < 0 ? -1 : 1;
            float* o = cov_f32 + 6 * (size_t)i;
            o[0] = (float)s3[0]; o[1] = (float)s3[1]; o[2] = 1.0f;
            for (int k = 0; k < 3; k++) o[3 + k] = (float)(q[k] * flip);
        } else if (!HOST || cov_f32 || cov_f16) {
            // Matrix4.makeRotationFromQuaternion = compose(zero, q, one) (three r160)
            const double x2 = x + x, y2 = y + y, z2 = z + z;
            const double xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2;
            const double wx = w * x2, wy = w * y2, wz = w * z2;
            const double R[3][3] = {{(1 - (yy + zz)) * 1, (xy - wz) * 1, (xz + wy) * 1},
                                    {(xy + wz) * 1, (1 - (xx + zz)) * 1, (yz - wx) * 1},
                                    {(xz - wy) * 1, (yz + wx) * 1, (1 - (xx + yy)) * 1}};
            // covarianceMatrix = R * S (Matrix3.multiplyMatrices: a_i1*b_1j + a_i2*b_2j + a_i3*b_3j)
            const double S[3][3] = {{sx, 0, 0}, {0, sy, 0}, {0, 0, sz}};
            double M[3][3], Cm[3][3];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = 0; q < 3; q++) M[r][q] = R[r][0] * S[0][q] + R[r][1] * S[1][q] + R[r][2] * S[2][q];
            // transformedCovariance = M * M^T
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = 0; q < 3; q++) Cm[r][q] = M[r][0] * M[q][0] + M[r][1] * M[q][1] + M[r][2] * M[q][2];
            double e[6] = {Cm[0][0], Cm[0][1], Cm[0][2], Cm[1][1], Cm[1][2], Cm[2][2]};   // elements 0,3,6,4,7,8
            if constexpr (XF) xf_covariance(t, Cm, e);                                     // T3 * C * T3^T (SplatBuffer.js:461-466)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                if (cov_f32) cov_f32[6 * (size_t)i + k] = XF ? xf_f32(e[k]) : (float)e[k];
                if (HOST ? cov_f16 != nullptr : !cov_f32) cov_f16[6 * (size_t)i + k] = XF ? xf_f16(e[k]) : to_half_three(e[k]);
            }
        }
    }
    if (!HOST || rgba) {   // fillSplatColorArray (SplatBuffer.js:551-575)
        const uint32_t word = row.colour(), alpha = word >> 24;
        const uint32_t out = (word & 0x00FFFFFFu) | ((alpha >= min_alpha ? alpha : 0u) << 24);
        __builtin_memcpy(rgba + sizeof(out) / sizeof(Rgba) * (size_t)i, &out, sizeof(out));   // the bytes R, G, B, A
    }
    const bool sh = ncomp && (!HOST || sh_f16 || sh_u8);
    if constexpr (XF) {   // fillSphericalHarmonicsArray with a transform: widened, rotated, converted from level 0
        if (sh)
            xf_sh(t, sh_degree, [&](uint32_t src) { return row.sh_wide(src, sh_lo, sh_hi); }, [&](uint32_t dst, double val) {
                if (sh_u8) sh_u8[(size_t)ncomp * i + dst] = to_uint8_range(val, sh_lo, sh_hi);
                else sh_f16[(size_t)ncomp * i + dst] = xf_f16(val);
            });
    } else if (sh) {   // ... without one: level 0 through the half rule, level 1 bits, level 2 bytes
        auto emit = [&](uint32_t dst, uint32_t src) {
            if (sh_u8) sh_u8[(size_t)ncomp * i + dst] = row.sh_byte(src);
            else sh_f16[(size_t)ncomp * i + dst] = row.sh_half(src);
        };
        for (uint32_t q = 0; q < 3; q++)                                                   // set3FromArray(stride 3, base c)
            for (uint32_t ch = 0; ch < 3; ch++) emit(3 * q + ch, q + 3 * ch);
        if (sh_degree >= 2)
            for (uint32_t q = 0; q < 5; q++)                                               // set3FromArray(stride 5, base 9 + c)
                for (uint32_t ch = 0; ch < 3; ch++) emit(9 + 3 * q + ch, 9 + q + 5 * ch);
    }
}

constexpr uint32_t GS_DEBUG_ASSET_ROW_BYTES = 140;         // what gs_debug_asset_row (assets.hip) writes at most: 44 + 4 * 24
enum AssetRows : uint32_t { ASSET_ROWS_KSPLAT = 0, ASSET_ROWS_SPLAT = 1, ASSET_ROWS_COMPRESSED_PLY = 2, ASSET_ROWS_SPZ = 3, ASSET_ROWS_INRIA_V2 = 4,
                            ASSET_ROWS_INRIA_V1 = 5 };

struct gs_asset {
    std::vector<uint8_t> buf;              // a .ksplat image (for an INRIA-v1 PLY: the level-0 section built from it; for the
                                           // row formats: built from `file` when a host fill first needs it)
    uint32_t rows = ASSET_ROWS_KSPLAT;     // what the device decode reads: the image, or the file's own rows
    std::vector<uint8_t> file;             // .splat / compressed / INRIA-v2 PLY: the file as it was given; .spz: the INFLATED stream
    SpzLayout spz = {};                    // .spz: where the planes lie in `file`
    PcLayout pc = {};                      // compressed PLY: the header's layout
    size_t pc_chunk_base = 0, pc_vertex_base = 0, pc_sh_base = 0;   // where the three elements start in `file`
    uint32_t pc_chunk_count = 0;
    InriaV2Layout iv2 = {};                // INRIA-v2 PLY: the vertex element's layout, where its rows start in `file`, and the
    size_t iv2_vertex_base = 0;            // codebook decoded at open (IV2_PAGES x 256 floats)
    std::vector<float> iv2_codebook;
    InriaV1Layout iv1 = {};                // a STREAMED INRIA-v1 PLY: the vertex element's layout and where its rows start in `file`
    size_t iv1_vertex_base = 0;            // (gs_asset_open lays a whole INRIA-v1 file out as a level-0 image instead)
    std::unique_ptr<AssetStream> stream;   // gs_asset_open_stream: the state of the stream (asset_stream.hpp), else null
    uint32_t level = 0, splat_count = 0, sh_degree = 0;
    float scene_center[3] = {0, 0, 0};
    double sh_min = -1.5, sh_max = 1.5;
    std::vector<KsplatSection> sections;   // of `buf`: the non-empty ones, offsets from buf's byte 0
    std::vector<uint32_t> partial_end;     // ... and the partial bucket ends of all of them
    bool has_transform = false;            // gs_asset_set_transform
    AssetTransform xf = {};
    bool encoded = false;                  // `buf` is a file image gs_asset_encode_ksplat made (gs_asset_bytes hands it out)
    // the splats an upload may name: all of an opened asset, the ready prefix of a stream
    uint32_t ready() const { return stream ? stream->splats_ready : splat_count; }
    bool incomplete() const { return stream && !stream->complete; }

    template <class T>
    T rd(size_t off) const {
        T v;
        memcpy(&v, buf.data() + off, sizeof(T));
        return v;
    }
    KsplatSource image() const {           // `buf` as a row source, at the asset's output SH degree
        KsplatSource v;
        v.image = buf.data();
        v.sections = sections.data();
        v.partial_end = partial_end.data();
        v.section_count = (uint32_t)sections.size();
        v.level = level;
        v.sh_degree = sh_degree;
        v.ncomp = sh_components(sh_degree);
        return v;
    }
};
