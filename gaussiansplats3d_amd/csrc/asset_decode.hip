// asset_decode.hip — the per-splat decode of an opened asset on the device: file rows -> the staging layout a
// mesh upload commits (gs_mesh_upload_asset) and the sorter's `centers` message (gs_sorter_upload_asset_centers).
// The kernels take a ROW SOURCE (a template parameter, as XF is one): the .ksplat image (also an INRIA-v1 PLY's level-0
// image), the 32-byte rows of a .splat, the 16-byte vertex rows + chunk rows + SH bytes of a PlayCanvas compressed PLY, or
// the six byte planes of an inflated .spz.  The last three produce the level-0 tuple in registers through asset_internal.hpp's
// row arithmetic - the functions the host's image builder calls - so only file rows cross the bus and the level-0 image is
// never built on this path.
// The arithmetic is gs_asset_fill's (assets.hip), expression for expression, in fp64 and unfused (this file is built with
// -ffp-contract=off): only multiplies, adds and double -> float conversions are involved, so the planes are bit-equal to what
// gs_asset_fill + gs_mesh_upload (+ gs_mesh_upload_sh_u8) leave.  Restates, never copies:
//   bucket of a splat / centre   /root/reference/src/loaders/SplatBuffer.js:199-246
//   covariance                   SplatBuffer.js:440-486, 517-549 (three.js Matrix3/4 arithmetic in double)
//   colour, SH order             SplatBuffer.js:551-575, 577-734
//   static scene transform       SplatBuffer.js:340-342, 461-466, 684-688, 707-715, 736-770 (the XF instantiations: an asset
//                                with gs_asset_set_transform; asset_internal.hpp says the arithmetic once for both sides)
//   integer centres              /root/reference/src/splatmesh/SplatMesh.js:1912-1948
// Header and section parsing stay host code (assets.hip); the device sees a section table and searches it per splat.
#include <algorithm>

#include "asset_internal.hpp"

namespace {

struct DevSection {
    long long data_off;        // byte offset of the section's row 0 in the device image (negative when the range starts inside the
                               // section: rows before the range are not uploaded)
    long long buckets_off;     // ... of its bucket centres
    uint32_t count_offset, count;
    uint32_t bytes_per_splat, bucket_size, full_buckets, bucket_count, bucket_storage, scale_range;
    uint32_t partial_begin, partial_count;   // its slice of the cumulative partial_end list behind the sections
    double scale_factor;
};

struct AssetView {             // kernel argument: the staged image
    const uint8_t* image;
    const DevSection* sections;
    const uint32_t* partial_end;
    uint32_t section_count, level, sh_degree, ncomp;
};

template <class T>
__device__ __forceinline__ T ld(const uint8_t* p) {            // rows have no alignment (33 bytes per splat at level 2, SH 1)
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// dataViewFloatForCompressionLevel for scale / rotation (never the 8-bit SH rule)
__device__ __forceinline__ double comp(uint32_t level, const uint8_t* row, uint32_t index) {
    if (level == 0) return (double)ld<float>(row + 4 * index);
    return from_half(ld<uint16_t>(row + 2 * index));
}

// the section of splat i: the last one that begins at or before it (the table holds the non-empty sections of the range in order)
__device__ __forceinline__ const DevSection& section_of(const AssetView& v, uint32_t i) {
    uint32_t lo = 0, hi = v.section_count;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.sections[mid].count_offset <= i) lo = mid;
        else hi = mid;
    }
    return v.sections[lo];
}

// SplatBuffer.js:199-219: full buckets first, then the partial ones by their stored lengths (std::upper_bound of the host)
__device__ __forceinline__ uint32_t bucket_index(const AssetView& v, const DevSection& sec, uint32_t local) {
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
__device__ __forceinline__ void ksplat_centre(const AssetView& v, const DevSection& sec, uint32_t local, const uint8_t* row, double d[3]) {
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

// ---- row sources ---------------------------------------------------------------------------------------------------------
// A source is the kernel argument that says where splat i's values come from.  Its Row gives: the double centre, the doubles
// of scale and rotation (w, x, y, z) as the fills read them, the colour bytes, and the SH of file index `src` in each of the
// three forms the store needs (widened double for the rotated fill, half bits, the level-2 byte).
struct KsplatSource : AssetView {
    struct Row {
        const AssetView& v;
        const DevSection& sec;
        uint32_t local;
        const uint8_t* row;
        __device__ __forceinline__ const uint8_t* srow() const { return row + asset_center_bytes(v.level); }
        __device__ __forceinline__ const uint8_t* crow() const { return srow() + asset_center_bytes(v.level) + asset_rotation_bytes(v.level); }
        __device__ __forceinline__ void centre(double d[3]) const { ksplat_centre(v, sec, local, row, d); }
        __device__ __forceinline__ void scale_rotation(double s[3], double q[4]) const {
            for (int k = 0; k < 3; k++) s[k] = comp(v.level, srow(), k);
            for (int k = 0; k < 4; k++) q[k] = comp(v.level, srow(), 3 + k);
        }
        __device__ __forceinline__ uint32_t colour() const { return ld<uint32_t>(crow()); }
        __device__ __forceinline__ double sh_wide(uint32_t src, double lo, double hi) const { return sh_widen(v.level, crow() + 4, src, lo, hi); }
        __device__ __forceinline__ uint16_t sh_half(uint32_t src) const {      // level 0 through the half rule, level 1 bits
            return v.level == 0 ? to_half_three((double)ld<float>(crow() + 4 + 4 * src)) : ld<uint16_t>(crow() + 4 + 2 * src);
        }
        __device__ __forceinline__ uint8_t sh_byte(uint32_t src) const { return crow()[4 + src]; }
    };
    __device__ __forceinline__ Row row(uint32_t splat) const {
        const DevSection& sec = section_of(*this, splat);
        const uint32_t local = splat - sec.count_offset;
        return Row{*this, sec, local, image + sec.data_off + (long long)sec.bytes_per_splat * local};
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const { row(splat).centre(d); }
};

// the level-0 tuple in registers, as the row formats produce it (fp32 values of a level-0 row, widened as the fills widen them)
struct TupleValues {
    Level0Tuple t;
    __device__ __forceinline__ void centre(double d[3]) const { for (int k = 0; k < 3; k++) d[k] = t.c[k]; }
    __device__ __forceinline__ void scale_rotation(double s[3], double q[4]) const {
        for (int k = 0; k < 3; k++) s[k] = t.s[k];
        for (int k = 0; k < 4; k++) q[k] = t.r[k];
    }
    __device__ __forceinline__ uint32_t colour() const {
        return (uint32_t)t.rgba[0] | ((uint32_t)t.rgba[1] << 8) | ((uint32_t)t.rgba[2] << 16) | ((uint32_t)t.rgba[3] << 24);
    }
};
struct TupleRow : TupleValues {
    const uint8_t* sh;             // compressed PLY: the splat's SH bytes (unaligned: 9 / 24 / 45 per splat)
    uint32_t read_coeff;
    __device__ __forceinline__ double sh_wide(uint32_t src, double, double) const { return (double)pc_row_sh(sh, read_coeff, src); }
    __device__ __forceinline__ uint16_t sh_half(uint32_t src) const { return to_half_three((double)pc_row_sh(sh, read_coeff, src)); }
    __device__ __forceinline__ uint8_t sh_byte(uint32_t) const { return 0; }       // sh_level is 1: never stored as bytes
};

// .splat: rows start at the allocation-aligned staging base, so a 32-byte row is two 16-byte loads
struct SplatSource {
    const uint4* rows;             // row 0 = asset splat `base`
    uint32_t base;
    uint32_t level, sh_degree, ncomp;   // 0, 0, 0
    using Row = TupleRow;
    __device__ __forceinline__ Row row(uint32_t splat) const {
        const uint4 a = rows[2 * (size_t)(splat - base)], b = rows[2 * (size_t)(splat - base) + 1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        Row r;
        splat_row_tuple(w, r.t);
        r.sh = nullptr;
        r.read_coeff = 0;
        return r;
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const {    // the first three floats of the row
        const uint4 a = rows[2 * (size_t)(splat - base)];
        d[0] = __builtin_bit_cast(float, a.x); d[1] = __builtin_bit_cast(float, a.y); d[2] = __builtin_bit_cast(float, a.z);
    }
};

// compressed PLY: one 16-byte load per vertex row; the chunk of a splat is floor(i / 256) by ABSOLUTE splat index, so a
// workgroup of 256 consecutive splats touches at most two chunk rows; the chunk rows keep their file stride and order
struct CompressedSource {
    const uint4* vertex;           // row 0 = asset splat `base`
    const uint8_t* chunks;         // row 0 = chunk base / 256
    const uint8_t* sh;             // row 0 = asset splat `base`
    uint32_t base;
    uint32_t level, sh_degree, ncomp;   // 0, the output degree, 0 / 9 / 24
    PcLayout layout;
    using Row = TupleRow;
    __device__ __forceinline__ const uint8_t* chunk_of(uint32_t splat) const {
        return chunks + (size_t)layout.chunk_stride * (splat / 256u - base / 256u);
    }
    __device__ __forceinline__ Row row(uint32_t splat) const {
        const uint4 a = vertex[splat - base];
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
        Row r;
        pc_row_tuple(w, chunk_of(splat), layout, r.t);
        r.sh = sh + (size_t)layout.sh_stride * (splat - base);
        r.read_coeff = layout.read_coeff;
        return r;
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const {    // the position word and six extremes only
        const uint32_t* words = reinterpret_cast<const uint32_t*>(vertex + (splat - base));
        float c[3];
        pc_row_centre(words[layout.word[0]], chunk_of(splat), layout, c);
        for (int k = 0; k < 3; k++) d[k] = c[k];
    }
};

// .spz: six byte planes.  A staged plane slice begins 16-byte aligned at asset splat `base`, whatever `base` is, so splat
// base + i has its bytes at stride * i - at any byte phase of a dword (strides 9 / 6 / 1 / 3 / 3 * dim).  There are no byte-wide
// global loads: a value is cut with shifts out of the aligned dword(s) that hold it; neighbouring lanes meet in the same dwords
// through the cache.  A second dword is loaded only when the value's own bytes reach into it, so the last lanes read at most
// the slice's padding to 16 bytes, never past the allocation (and whatever the padding holds is masked away).
__device__ __forceinline__ uint32_t spz_load1(const uint32_t* words, size_t b) { return (words[b >> 2] >> (8u * (uint32_t)(b & 3u))) & 255u; }
__device__ __forceinline__ uint32_t spz_load2(const uint32_t* words, size_t b) {       // b is even: one dword holds both bytes
    return (words[b >> 2] >> (8u * (uint32_t)(b & 3u))) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t spz_load3(const uint32_t* words, size_t b) {
    const uint32_t shift = 8u * (uint32_t)(b & 3u);
    uint32_t v = words[b >> 2] >> shift;
    if (shift > 8u) v |= words[(b >> 2) + 1] << (32u - shift);                         // phases 2 and 3 continue in the next dword
    return v & 0x00FFFFFFu;
}

struct SpzSource {
    const uint32_t* plane[SPZ_PLANES];   // byte 0 of each slice = asset splat `base` (SH: staged whole, 3 * file_dim per splat)
    uint32_t base;
    uint32_t level, sh_degree, ncomp;    // 0, the output degree, 0 / 9 / 24
    SpzLayout layout;
    struct Row : TupleValues {
        const uint32_t* sh;              // the SH slice
        size_t sh_at;                    // byte offset of this splat's SH in it
        __device__ __forceinline__ float value(uint32_t src) const { return spz_sh_value(spz_load1(sh, sh_at + spz_sh_index(src))); }
        __device__ __forceinline__ double sh_wide(uint32_t src, double, double) const { return (double)value(src); }
        __device__ __forceinline__ uint16_t sh_half(uint32_t src) const { return to_half_three((double)value(src)); }
        __device__ __forceinline__ uint8_t sh_byte(uint32_t) const { return 0; }   // sh_level is 1: never stored as bytes
    };
    __device__ __forceinline__ void positions(size_t i, uint32_t pos[3]) const {
        for (int k = 0; k < 3; k++)
            pos[k] = layout.pos_stride == 9u ? spz_load3(plane[SPZ_POSITIONS], 9 * i + 3 * k) : spz_load2(plane[SPZ_POSITIONS], 6 * i + 2 * k);
    }
    __device__ __forceinline__ Row row(uint32_t splat) const {
        const size_t i = splat - base;
        SpzRowBytes b;
        positions(i, b.pos);
        b.alpha = spz_load1(plane[SPZ_ALPHAS], i);
        b.colour = spz_load3(plane[SPZ_COLOURS], 3 * i);
        b.scale = spz_load3(plane[SPZ_SCALES], 3 * i);
        b.rotation = spz_load3(plane[SPZ_ROTATIONS], 3 * i);
        Row r;
        spz_row_tuple(layout, b, r.t);
        r.sh = plane[SPZ_SH];
        r.sh_at = 3 * (size_t)layout.file_dim * i;
        return r;
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const {    // the position plane alone
        uint32_t pos[3];
        float c[3];
        positions(splat - base, pos);
        spz_row_centre(layout, pos, c);
        for (int k = 0; k < 3; k++) d[k] = c[k];
    }
};

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

// the double centre through the scene transform (SplatBuffer.js:332-342) or narrowed to float as fillSplatCenterArray stores it
template <bool XF>
__device__ __forceinline__ void store_centre(const AssetTransform& t, const double d[3], float c[3]) {
    if constexpr (XF) xf_centre(t, d, c);
    else for (int k = 0; k < 3; k++) c[k] = (float)d[k];
}

// One thread per splat: asset splat first + i -> element i of the staging arrays (MeshStaging).
template <class Source, bool XF, class Transform>
__global__ __launch_bounds__(256) void k_asset_decode(Source v, Transform xf, uint32_t first, uint32_t count, uint32_t min_alpha,
                                                      float* __restrict__ centers, float* __restrict__ cov_f32,
                                                      uint16_t* __restrict__ cov_f16, uint32_t* __restrict__ rgba,
                                                      uint16_t* __restrict__ sh_f16, uint8_t* __restrict__ sh_u8) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const AssetTransform& t = transform_of(xf);
    const typename Source::Row row = v.row(first + i);
    {
        double d[3];
        float c[3];
        row.centre(d);
        store_centre<XF>(t, d, c);
        for (int k = 0; k < 3; k++) centers[3 * (size_t)i + k] = c[k];
    }
    {
        double s3[3], q4[4];
        row.scale_rotation(s3, q4);
        const double sx = s3[0], sy = s3[1], sz = s3[2];
        // rotation.set(x = f4, y = f5, z = f6, w = f3): NOT normalised (SplatBuffer.js:539-542)
        const double w = q4[0], x = q4[1], y = q4[2], z = q4[3];
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
            else cov_f16[6 * (size_t)i + k] = XF ? xf_f16(e[k]) : to_half_three(e[k]);
        }
    }
    {   // fillSplatColorArray (SplatBuffer.js:551-575)
        const uint32_t word = row.colour(), alpha = word >> 24;
        rgba[i] = (word & 0x00FFFFFFu) | ((alpha >= min_alpha ? alpha : 0u) << 24);
    }
    if constexpr (XF) {   // fillSphericalHarmonicsArray with a transform: widened, rotated, converted from level 0
        if (v.ncomp)
            xf_sh(t, v.sh_degree, [&](uint32_t src) { return row.sh_wide(src, sh_lo(xf), sh_hi(xf)); }, [&](uint32_t dst, double val) {
                if (sh_u8) sh_u8[(size_t)v.ncomp * i + dst] = to_uint8_range(val, sh_lo(xf), sh_hi(xf));
                else sh_f16[(size_t)v.ncomp * i + dst] = xf_f16(val);
            });
    } else if (v.ncomp) {   // ... without one: level 0 through the half rule, level 1 bits, level 2 bytes
        auto emit = [&](uint32_t dst, uint32_t src) {
            if (sh_u8) sh_u8[(size_t)v.ncomp * i + dst] = row.sh_byte(src);
            else sh_f16[(size_t)v.ncomp * i + dst] = row.sh_half(src);
        };
        for (uint32_t q = 0; q < 3; q++)                                               // set3FromArray(stride 3, base c)
            for (uint32_t ch = 0; ch < 3; ch++) emit(3 * q + ch, q + 3 * ch);
        if (v.sh_degree >= 2)
            for (uint32_t q = 0; q < 5; q++)                                           // set3FromArray(stride 5, base 9 + c)
                for (uint32_t ch = 0; ch < 3; ch++) emit(9 + 3 * q + ch, 9 + q + 5 * ch);
    }
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

// Uploads what the kernels read of splats [first, first + count), count > 0, in range: their rows (one contiguous piece of the
// file), the bucket tables of their sections and the section table.  Synchronises `st`: the host table is a local.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, KsplatSource* view, bool /*centres_only*/) {
    const uint32_t last = first + count - 1u;
    std::vector<DevSection> table;
    std::vector<uint32_t> partial;
    std::vector<const AssetSection*> used;
    for (const AssetSection& sec : a->sections) {
        if (sec.max_splat_count == 0 || sec.count_offset > last || sec.count_offset + sec.max_splat_count <= first) continue;
        used.push_back(&sec);
    }
    GS_REQUIRE(!used.empty(), "the asset has no section for the range");
    const AssetSection &sa = *used.front(), &sb = *used.back();
    const size_t lo = sa.data_base + (size_t)sa.bytes_per_splat * (first - sa.count_offset);
    const size_t hi = sb.data_base + (size_t)sb.bytes_per_splat * (last - sb.count_offset + 1u);
    size_t bytes = (hi - lo + 15) & ~(size_t)15;
    for (const AssetSection* sec : used) {
        DevSection d = {};
        d.data_off = (long long)sec->data_base - (long long)lo;
        d.count_offset = sec->count_offset;
        d.count = sec->max_splat_count;
        d.bytes_per_splat = sec->bytes_per_splat;
        d.bucket_size = sec->bucket_size;
        d.full_buckets = sec->full_buckets;
        d.bucket_count = sec->bucket_count;
        d.bucket_storage = sec->bucket_storage;
        d.scale_range = sec->scale_range;
        d.scale_factor = sec->scale_factor;
        d.partial_begin = (uint32_t)partial.size();
        d.partial_count = (uint32_t)sec->partial_end.size();
        partial.insert(partial.end(), sec->partial_end.begin(), sec->partial_end.end());
        if (a->level > 0) {                                  // bucket tables are only read for compressed centres
            d.buckets_off = (long long)bytes;
            bytes += ((size_t)sec->bucket_storage * sec->bucket_count + 15) & ~(size_t)15;
        }
        table.push_back(d);
    }
    const size_t table_bytes = table.size() * sizeof(DevSection), partial_bytes = partial.size() * 4;
    GS_TRY(dev.bytes.ensure(bytes));
    GS_TRY(dev.table.ensure(table_bytes + partial_bytes + 16));
    uint8_t* image = dev.bytes.as<uint8_t>();
    GS_HIP(hipMemcpyAsync(image, a->buf.data() + lo, hi - lo, hipMemcpyHostToDevice, st));
    if (a->level > 0)
        for (size_t k = 0; k < used.size(); k++)
            if (used[k]->bucket_count)
                GS_HIP(hipMemcpyAsync(image + table[k].buckets_off, a->buf.data() + used[k]->buckets_base,
                                      (size_t)used[k]->bucket_storage * used[k]->bucket_count, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(dev.table.p, table.data(), table_bytes, hipMemcpyHostToDevice, st));
    if (partial_bytes) GS_HIP(hipMemcpyAsync(dev.table.as<char>() + table_bytes, partial.data(), partial_bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    view->image = image;
    view->sections = dev.table.as<DevSection>();
    view->partial_end = reinterpret_cast<const uint32_t*>(dev.table.as<char>() + table_bytes);
    view->section_count = (uint32_t)table.size();
    view->level = a->level;
    view->sh_degree = a->sh_degree;
    view->ncomp = sh_components(a->sh_degree);
    return GS_OK;
}

// .splat: rows [first, first + count) at the staging base
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, SplatSource* src, bool /*centres_only*/) {
    const size_t bytes = 32 * (size_t)count;
    GS_TRY(dev.bytes.ensure(bytes));
    GS_HIP(hipMemcpyAsync(dev.bytes.p, a->file.data() + 32 * (size_t)first, bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    *src = SplatSource{dev.bytes.as<uint4>(), first, 0u, 0u, 0u};
    return GS_OK;
}

// compressed PLY: the range's 16-byte vertex rows, the chunk rows first / 256 .. (first + count - 1) / 256 at their file stride,
// and - unless only centres are wanted - the range's SH rows (one splat's bytes are contiguous in the file); each piece starts
// 16-byte aligned.  gs_asset_open
// proved that the file holds all three.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, CompressedSource* src,
                bool centres_only) {
    const uint32_t chunk_lo = first / 256u, chunk_hi = (first + count - 1u) / 256u;
    const uint32_t ncomp = sh_components(a->sh_degree);
    const size_t vertex_bytes = 16 * (size_t)count, chunk_bytes = (size_t)a->pc.chunk_stride * (chunk_hi - chunk_lo + 1u),
                 sh_bytes = ncomp && !centres_only ? (size_t)a->pc.sh_stride * count : 0;
    const size_t chunk_off = vertex_bytes, sh_off = chunk_off + ((chunk_bytes + 15) & ~(size_t)15);
    GS_TRY(dev.bytes.ensure(sh_off + ((sh_bytes + 15) & ~(size_t)15)));
    uint8_t* image = dev.bytes.as<uint8_t>();
    GS_HIP(hipMemcpyAsync(image, a->file.data() + a->pc_vertex_base + 16 * (size_t)first, vertex_bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(image + chunk_off, a->file.data() + a->pc_chunk_base + (size_t)a->pc.chunk_stride * chunk_lo, chunk_bytes,
                          hipMemcpyHostToDevice, st));
    if (sh_bytes)
        GS_HIP(hipMemcpyAsync(image + sh_off, a->file.data() + a->pc_sh_base + (size_t)a->pc.sh_stride * first, sh_bytes,
                              hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    *src = CompressedSource{reinterpret_cast<const uint4*>(image), image + chunk_off, image + sh_off, first, 0u, a->sh_degree, ncomp, a->pc};
    return GS_OK;
}

// .spz: the slices [first, first + count) of the six planes (the position plane alone for the sorter's centres), each starting
// 16-byte aligned and padded to 16 bytes; nothing else crosses the bus (19 + 3 * file_dim bytes per splat for version 2).  The SH
// of a degree-3 file is staged whole and read up to the output degree.  spz_open proved that the stream holds every plane.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, SpzSource* src, bool centres_only) {
    const SpzLayout& L = a->spz;
    const uint32_t ncomp = sh_components(a->sh_degree);
    size_t at[SPZ_PLANES], bytes[SPZ_PLANES], total = 0;
    for (int p = 0; p < SPZ_PLANES; p++) {
        const bool wanted = p == SPZ_POSITIONS || (!centres_only && (p != SPZ_SH || ncomp));
        at[p] = total;
        bytes[p] = wanted ? (size_t)spz_plane_stride(L, p) * count : 0;
        total += (bytes[p] + 15) & ~(size_t)15;
    }
    GS_TRY(dev.bytes.ensure(total));
    uint8_t* image = dev.bytes.as<uint8_t>();
    for (int p = 0; p < SPZ_PLANES; p++)
        if (bytes[p])
            GS_HIP(hipMemcpyAsync(image + at[p], a->file.data() + L.off[p] + (size_t)spz_plane_stride(L, p) * first, bytes[p],
                                  hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    SpzSource v = {};
    for (int p = 0; p < SPZ_PLANES; p++) v.plane[p] = reinterpret_cast<const uint32_t*>(image + at[p]);
    v.base = first;
    v.level = 0;
    v.sh_degree = a->sh_degree;
    v.ncomp = ncomp;
    v.layout = L;
    *src = v;
    return GS_OK;
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
        if (asset->has_transform)
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
    GS_REQUIRE((uint64_t)first + count <= a->splat_count, "range exceeds the asset's splat count");
    GS_REQUIRE(m->sh_degree == a->sh_degree, "the mesh's SH degree differs from the asset's (gs_asset_info.sh_degree)");
    const bool mesh_u8 = (m->flags & GS_MESH_SH_U8) != 0;
    GS_REQUIRE(m->sh_degree == 0 || mesh_u8 == (a->level == 2),
               "GS_MESH_SH_U8 must be set exactly for a file whose SH are uint8 (gs_asset_info.sh_level == 2)");
    if (count == 0) return GS_OK;
    ScopedDevice sd(m->ctx->device);
    // (an earlier call's decode kernels have finished: every upload synchronises before it returns)
    if (a->rows == ASSET_ROWS_SPLAT) return mesh_upload_rows<SplatSource>(m, from, a, first, count, min_alpha, mesh_u8);
    if (a->rows == ASSET_ROWS_COMPRESSED_PLY) return mesh_upload_rows<CompressedSource>(m, from, a, first, count, min_alpha, mesh_u8);
    if (a->rows == ASSET_ROWS_SPZ) return mesh_upload_rows<SpzSource>(m, from, a, first, count, min_alpha, mesh_u8);
    return mesh_upload_rows<KsplatSource>(m, from, a, first, count, min_alpha, mesh_u8);
}

int gs_sorter_upload_asset_centers(gs_sorter* s, uint32_t from, gs_asset* a, uint32_t first, uint32_t count,
                                   const uint32_t* scene_indexes) {
    GS_REQUIRE(s && a, "sorter / asset == NULL");
    GS_REQUIRE((uint64_t)from + count <= s->max_count, "range exceeds max_splat_count");
    GS_REQUIRE((uint64_t)first + count <= a->splat_count, "range exceeds the asset's splat count");
    GS_REQUIRE(!(s->flags & GS_SORT_DYNAMIC) || scene_indexes, "dynamic sorter needs scene_indexes");
    GS_REQUIRE(!(s->flags & GS_SORT_DYNAMIC) || !a->has_transform,
               "a dynamic sorter takes untransformed centres: dynamic mode applies scene transforms per frame and never bakes them");
    if (count == 0) return GS_OK;
    ScopedDevice sd(s->ctx->device);
    if (a->rows == ASSET_ROWS_SPLAT) GS_TRY(sorter_upload_rows<SplatSource>(s, from, a, first, count));
    else if (a->rows == ASSET_ROWS_COMPRESSED_PLY) GS_TRY(sorter_upload_rows<CompressedSource>(s, from, a, first, count));
    else if (a->rows == ASSET_ROWS_SPZ) GS_TRY(sorter_upload_rows<SpzSource>(s, from, a, first, count));
    else GS_TRY(sorter_upload_rows<KsplatSource>(s, from, a, first, count));
    return gs_sorter_commit_centers(s, from, count, scene_indexes);
}

}  // extern "C"
