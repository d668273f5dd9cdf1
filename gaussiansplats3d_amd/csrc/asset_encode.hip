// asset_encode.hip — an opened level-0 asset -> a one-section .ksplat image (compression levels 0 / 1 / 2) on the device:
// gs_asset_encode_ksplat.  The result is byte for byte what SplatBuffer.generateFromUncompressedSplatArrays returns for the
// asset's level-0 rows in file order.  Restates, never copies:
//   drop, SH range, section and file layout   src/loaders/SplatBuffer.js:1177-1326
//   buckets                                    src/loaders/SplatBuffer.js:1328-1399 (computeBucketsForUncompressedSplatArray)
//   a row                                      src/loaders/SplatBuffer.js:1050-1175 (writeSplatDataToSectionBuffer)
//   headers                                    src/loaders/SplatBuffer.js:856-875, 944-960
// The reference's bucket bookkeeping is a sequential loop over a hash map keyed by cell id.  Its data-parallel form: a stable
// sort of the kept splats by cell id puts a cell's splats side by side in file order; the rank of a splat inside its cell says
// which of the cell's buckets it is in (rank / bucket_size) and whether that bucket filled; a full bucket closed when its last
// member was read, so the full buckets are ordered by that member's kept position; the open ones follow by cell id, which is
// the sorted order already (`for ... in` walks integer keys in ascending order).
// The kernels, in launch order (Source = a row source of asset_sources.hpp; only file rows cross the bus):
//   k_enc_flags<Source>     per source row: keep flag (alpha >= min_alpha); min / max of the kept centres; the SH range's plain
//                           part (the least strictly negative and the greatest strictly positive value of FRC0..22, all rows)
//   k_cmp_count, k_scan_excl, k_cmp_write   stable compaction of flagged positions (used for the kept rows and the bucket heads)
//   k_enc_cells<Source>     per kept splat: its cell id (fp64, unfused), the sort's key, with its kept position as the value
//   radix_pass x 4          radix.hpp's stable key + value pass, as the octree build uses it
//   k_enc_heads             per sorted position: rank in its cell by two binary searches; marks heads of full / open buckets
//   k_enc_close_keys        per full bucket: the kept position of its closing member (then a second 4-pass sort)
//   k_enc_buckets<Source>   per bucket in output order: length, centre from its first member, the bucket table and open lengths
//   k_enc_rows<Source>      per OUTPUT row: decodes its source row through the Row interface, encodes it into LDS; the workgroup
//                           then stores its 256 rows, contiguous in the file, as whole dwords
// The host assembles header, section header and the section (ksplat_layout says where everything lies).
#include <math.h>

#include "asset_sources.hpp"
#include "radix.hpp"

// ---- where the parts of the file lie: host only --------------------------------------------------------------------------------
// generateFromUncompressedSplatArrays :1234-1238, 1296-1322 for one section: header, section header, then the section: the open
// buckets' lengths (uint32 each), the bucket centres (3 floats each, full buckets first), the rows.  Level 0 stores no buckets.
struct gs_ksplat_layout {
    uint32_t bytes_per_splat, bucket_count;
    uint64_t partial_off, buckets_off, rows_off, storage_bytes, total_bytes;
};
static void ksplat_layout(uint32_t level, uint32_t sh_degree, uint32_t kept, uint32_t full, uint32_t partial, gs_ksplat_layout* out) {
    gs_ksplat_layout l = {};
    l.bytes_per_splat = asset_center_bytes(level) + asset_scale_bytes(level) + asset_rotation_bytes(level) + 4u +
                        asset_sh_value_bytes(level) * sh_components(sh_degree);
    l.bucket_count = level >= 1 ? full + partial : 0u;
    const uint64_t base = 4096 + 1024;
    const uint64_t meta = level >= 1 ? 4ull * partial : 0ull, centres = 12ull * l.bucket_count;
    l.partial_off = base;
    l.buckets_off = base + meta;
    l.rows_off = base + meta + centres;
    l.storage_bytes = meta + centres + (uint64_t)l.bytes_per_splat * kept;
    l.total_bytes = base + l.storage_bytes;
    *out = l;
}
// Debug entry for the tests (pure host; not in the public header)
extern "C" int gs_debug_ksplat_layout(uint32_t level, uint32_t sh_degree, uint32_t kept, uint32_t full, uint32_t partial,
                                      gs_ksplat_layout* out) {
    GS_REQUIRE(out && level <= 2 && sh_degree <= 2, "gs_debug_ksplat_layout: out == NULL, level > 2 or degree > 2");
    ksplat_layout(level, sh_degree, kept, full, partial, out);
    return GS_OK;
}

// (its sibling for one row of a stream's ready prefix is gs_debug_asset_row, assets.hip: the readers it needs live there)
// Debug entry for the tests (not in the public header): the level-0 image the host readers lay an asset's rows out as - what the
// encoder's result is compared with through a host model.  Valid until the asset is closed.
extern "C" int gs_debug_asset_level0_image(gs_asset* a, const void** data, uint64_t* bytes) {
    GS_REQUIRE(a && data && bytes, "asset / data / bytes == NULL");
    GS_REQUIRE(a->level == 0, "the asset is no level-0 asset");
    GS_TRY(gs_asset_fill(a, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));   // builds it when rows are kept as a file
    *data = a->buf.data();
    *bytes = a->buf.size();
    return GS_OK;
}

namespace {

struct EncParams {
    double mn[3];              // exact minimum of the kept centres
    double block, half_block;  // blockSize, blockSize / 2.0
    double yz_blocks, z_blocks;   // yBlocks * zBlocks, zBlocks
    double scale_factor;       // compressionScaleRange / (blockSize * 0.5)
    double sh_lo, sh_hi;       // min / maxSphericalHarmonicsCoeff
    uint32_t level, ncomp, bytes_per_splat, bucket_size;
};

// order-preserving image of a finite float in uint32
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float ordered_float(uint32_t u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

enum { RED_MIN = 0, RED_MAX = 3, RED_SH_NEG = 6, RED_SH_POS = 7, RED_BAD = 8, RED_WORDS = 9 };
__device__ __forceinline__ uint32_t red_identity(uint32_t k) { return k < RED_MAX ? 0xFFFFFFFFu : 0u; }
__device__ __forceinline__ uint32_t red_join(uint32_t k, uint32_t a, uint32_t b) { return k < RED_MAX ? min(a, b) : max(a, b); }

// Per source row.  keep[i] = (alpha || 0) >= min_alpha (:1219).  red[RED_MIN / RED_MAX + k]: the extremes of the kept centres as
// ordered bits (:1335-1346; every kept centre is finite or RED_BAD is set and the call refuses).  The SH range (:1189-1202) is
// scanned over all rows and components FRC0 .. min(ncomp, 23) - 1; before the first strictly negative value its running minimum
// is never negative, that value replaces it whatever it is, and from there on `v < m` is a plain minimum - so whenever a strictly
// negative value exists the result is the least of them; likewise the greatest strictly positive one.  Those two leave as raw
// float bits (for one sign, raw bits order as magnitudes): 0 = none, and the host then walks the rule itself.
template <class Source>
__global__ __launch_bounds__(256) void k_enc_flags(Source v, uint32_t n, uint32_t min_alpha, uint32_t nscan, uint8_t* __restrict__ keep,
                                                   uint32_t* __restrict__ red) {
    __shared__ uint32_t s_red[RED_WORDS];
    if (threadIdx.x < RED_WORDS) s_red[threadIdx.x] = red_identity(threadIdx.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t r[RED_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < RED_WORDS; k++) r[k] = red_identity(k);
    if (i < n) {
        const auto row = v.row(i);
        const bool kept = (row.colour() >> 24) >= min_alpha;
        keep[i] = kept ? 1 : 0;
        if (kept) {
            double d[3];
            row.centre(d);
            for (int k = 0; k < 3; k++) {
                const float c = (float)d[k];
                if ((__builtin_bit_cast(uint32_t, c) & 0x7F800000u) == 0x7F800000u) r[RED_BAD] = 1u;
                else r[RED_MIN + k] = r[RED_MAX + k] = ordered_bits(c);
            }
        }
        for (uint32_t s = 0; s < nscan; s++) {
            const float f = (float)row.sh_wide(s, 0.0, 0.0);
            const uint32_t bits = __builtin_bit_cast(uint32_t, f);
            if (f < 0.0f) r[RED_SH_NEG] = max(r[RED_SH_NEG], bits);
            if (f > 0.0f) r[RED_SH_POS] = max(r[RED_SH_POS], bits);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < RED_WORDS; k++) {
        for (int o = 32; o > 0; o >>= 1) r[k] = red_join(k, r[k], (uint32_t)__shfl_xor((int)r[k], o, 64));
        if ((threadIdx.x & 63u) == 0 && r[k] != red_identity(k)) {
            if (k < RED_MAX) atomicMin(&s_red[k], r[k]);
            else atomicMax(&s_red[k], r[k]);
        }
    }
    __syncthreads();
    if (threadIdx.x < RED_WORDS && s_red[threadIdx.x] != red_identity(threadIdx.x)) {
        if (threadIdx.x < RED_MAX) atomicMin(&red[threadIdx.x], s_red[threadIdx.x]);
        else atomicMax(&red[threadIdx.x], s_red[threadIdx.x]);
    }
}

// ---- stable compaction: the positions j < n with kind[j] == match, ascending ------------------------------------------------------
__global__ __launch_bounds__(256) void k_cmp_count(const uint8_t* __restrict__ kind, uint32_t match, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const int c = __syncthreads_count(j < n && kind[j] == match);
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)c;
}
// exclusive prefix sums of data[0 .. n) in place, the sum to *total: ONE workgroup walks the array (a count per 256 elements, or
// a length per bucket: thousands of words)
__global__ __launch_bounds__(1024) void k_scan_excl(uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_tmp[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < n ? data[j] : 0u;
        uint32_t sum;
        const uint32_t ex = block_excl_scan<16>(v, s_tmp, &sum);
        if (j < n) data[j] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(256) void k_cmp_write(const uint8_t* __restrict__ kind, uint32_t match, uint32_t n,
                                                   const uint32_t* __restrict__ offsets, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_tmp[4];
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const bool on = j < n && kind[j] == match;
    const uint32_t ex = block_excl_scan_256(on ? 1u : 0u, s_tmp, nullptr);
    if (on) out[offsets[blockIdx.x] + ex] = j;
}

// the block of a centre along one axis (:1361-1363), an IEEE subtraction and division
__device__ __forceinline__ double block_of(double c, double mn, double block) {
#pragma clang fp contract(off)
    return floor((c - mn) / block);
}

// Per kept splat p (source row kept[p]): keys[p] = bucketId (:1369, below 2^32 - 1: the host checked the greatest one), vals[p] = p
template <class Source>
__global__ __launch_bounds__(256) void k_enc_cells(Source v, EncParams P, const uint32_t* __restrict__ kept, uint32_t count,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= count) return;
    double d[3];
    v.centre(kept[p], d);
    const double xb = block_of(d[0], P.mn[0], P.block), yb = block_of(d[1], P.mn[1], P.block), zb = block_of(d[2], P.mn[2], P.block);
    const double id = xb * P.yz_blocks + yb * P.z_blocks + zb;
    keys[p] = (uint32_t)id;
    vals[p] = p;
}

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t key) {   // first j with a[j] >= key
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound_u32(const uint32_t* a, uint32_t n, uint32_t key) {   // first j with a[j] > key
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

enum { HEAD_NONE = 0, HEAD_FULL = 1, HEAD_OPEN = 2 };
// Per position j of the sorted list: its rank in its cell = j - (first position of the cell).  A bucket begins at every rank that
// is a multiple of bucket_size (:1378-1382); it is full when the cell still holds bucket_size splats from there.
__global__ __launch_bounds__(256) void k_enc_heads(const uint32_t* __restrict__ sorted_keys, uint32_t count, uint32_t bucket_size,
                                                   uint8_t* __restrict__ kind) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint32_t key = sorted_keys[j];
    const uint32_t rank = j - lower_bound_u32(sorted_keys, count, key);
    uint8_t k = HEAD_NONE;
    if (rank % bucket_size == 0) k = upper_bound_u32(sorted_keys, count, key) - j >= bucket_size ? HEAD_FULL : HEAD_OPEN;
    kind[j] = k;
}

// Per full bucket f (head at sorted position heads[f]): the kept position of the member that closed it - the sort is stable, so
// a cell's members ascend - as the key of the second sort, the head as its value
__global__ __launch_bounds__(256) void k_enc_close_keys(const uint32_t* __restrict__ heads, uint32_t count, const uint32_t* __restrict__ sorted_vals,
                                                        uint32_t bucket_size, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= count) return;
    const uint32_t head = heads[f];
    keys[f] = sorted_vals[head + bucket_size - 1u];
    vals[f] = head;
}

// Per bucket b in output order (full ones by closing time, then the open ones; heads[b] = its first sorted position): its length,
// and its centre - the block centre of the splat that opened it (:1365-1375), which is its first member: xBlock * blockSize + min +
// halfBlockSize in doubles (kept for the rows' deltas), narrowed to the table's floats (:1265-1273); the open buckets' lengths (:1261-1264).
template <class Source>
__global__ __launch_bounds__(256) void k_enc_buckets(Source v, EncParams P, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ sorted_keys,
                                                     const uint32_t* __restrict__ sorted_vals, uint32_t count, const uint32_t* __restrict__ heads,
                                                     uint32_t buckets, uint32_t full, uint32_t* __restrict__ lengths, double* __restrict__ centres,
                                                     float* __restrict__ table, uint32_t* __restrict__ open_lengths) {
#pragma clang fp contract(off)
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= buckets) return;
    const uint32_t head = heads[b];
    const uint32_t len = b < full ? P.bucket_size : upper_bound_u32(sorted_keys, count, sorted_keys[head]) - head;
    lengths[b] = len;
    if (b >= full) open_lengths[b - full] = len;
    double d[3];
    v.centre(kept[sorted_vals[head]], d);
    for (int k = 0; k < 3; k++) {
        const double c = block_of(d[k], P.mn[k], P.block) * P.block + P.mn[k] + P.half_block;
        centres[3 * (size_t)b + k] = c;
        table[3 * (size_t)b + k] = (float)c;
    }
}

// `v || 0` of a number: NaN and both zeroes become +0
__device__ __forceinline__ double or_zero(double v) { return (v == v && v != 0.0) ? v : 0.0; }

template <class T>
__device__ __forceinline__ void put(uint8_t* o, T v) { __builtin_memcpy(o, &v, sizeof(T)); }

// writeSplatDataToSectionBuffer (:1075-1173) of one row into o (any byte phase).  bucket: the bucket's double centre (levels 1, 2).
template <class Row>
__device__ __forceinline__ void encode_row(const Row& row, const EncParams& P, const double* bucket, uint8_t* o) {
#pragma clang fp contract(off)
    double d[3], s[3], q[4];
    row.centre(d);
    row.scale_rotation(s, q);
    row_normalize(q);                                          // tempRot.set(ROT0..3).normalize() :1093-1094: x, y, z, w = the four slots
    for (int k = 0; k < 3; k++) s[k] = or_zero(s[k]);          // :1100-1102
    uint8_t* sh;
    if (P.level == 0) {
        for (int k = 0; k < 3; k++) put(o + 4 * k, (float)d[k]);
        for (int k = 0; k < 3; k++) put(o + 12 + 4 * k, (float)s[k]);
        for (int k = 0; k < 4; k++) put(o + 24 + 4 * k, row_f32(q[k]));
        put(o + 40, row.colour());
        sh = o + 44;
        for (uint32_t c = 0; c < P.ncomp; c++) put(sh + 4 * c, (float)or_zero(row.sh_wide(c, 0.0, 0.0)));
    } else {
        for (int k = 0; k < 3; k++) {                          // compressPositionOffset :1069-1073 of Vector3.sub :1133
            const double off = js_round((d[k] - bucket[k]) * P.scale_factor) + 32767.0;
            put(o + 2 * k, (uint16_t)clampd(off, 0.0, 65535.0));
        }
        for (int k = 0; k < 3; k++) put(o + 6 + 2 * k, to_half_three(s[k]));
        for (int k = 0; k < 4; k++) put(o + 12 + 2 * k, xf_f16(q[k]));
        put(o + 20, row.colour());
        sh = o + 24;
        for (uint32_t c = 0; c < P.ncomp; c++) {
            const double val = or_zero(row.sh_wide(c, 0.0, 0.0));
            if (P.level == 1) put(sh + 2 * c, to_half_three(val));
            else sh[c] = to_uint8_range(val, P.sh_lo, P.sh_hi);
        }
    }
}

constexpr uint32_t ENC_MAX_ROW = 140;     // level 0, degree 2: 44 + 4 * 24
// One thread per OUTPUT row r: its bucket by a search of the buckets' first rows, its place in the bucket, the sorted position,
// the kept position, the source row (order[r]).  The row is encoded into LDS; the workgroup's 256 rows are contiguous in the file
// and begin at a multiple of 256 * bytes_per_splat bytes of `rows` (a 4-byte multiple), so they leave as whole dwords; the last
// workgroup's odd bytes go one by one.
template <class Source>
__global__ __launch_bounds__(256) void k_enc_rows(Source v, EncParams P, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ sorted_vals,
                                                  const uint32_t* __restrict__ heads, const uint32_t* __restrict__ first_row, uint32_t buckets,
                                                  const double* __restrict__ centres, uint32_t count, uint8_t* __restrict__ rows,
                                                  uint32_t* __restrict__ order) {
    __shared__ __align__(16) uint32_t s_rows[256u * ENC_MAX_ROW / 4u];
    const uint32_t r0 = blockIdx.x * 256u, r = r0 + threadIdx.x;
    if (r < count) {
        const uint32_t b = upper_bound_u32(first_row, buckets, r) - 1u;          // first_row[0] == 0 <= r
        const uint32_t i = kept[sorted_vals[heads[b] + (r - first_row[b])]];
        order[r] = i;
        encode_row(v.row(i), P, centres + 3 * (size_t)b, reinterpret_cast<uint8_t*>(s_rows) + (size_t)P.bytes_per_splat * threadIdx.x);
    }
    __syncthreads();
    const uint32_t here = min(256u, count - r0), bytes = here * P.bytes_per_splat;
    uint8_t* dst = rows + (size_t)r0 * P.bytes_per_splat;
    for (uint32_t w = threadIdx.x; w < bytes / 4u; w += 256u) reinterpret_cast<uint32_t*>(dst)[w] = s_rows[w];
    if (threadIdx.x < (bytes & 3u)) dst[(bytes & ~3u) + threadIdx.x] = reinterpret_cast<const uint8_t*>(s_rows)[(bytes & ~3u) + threadIdx.x];
}

uint32_t grid_of(uint32_t n) { return (n + 255u) / 256u; }

// what one encode holds on the device
struct EncodeBuffers {
    AssetDeviceImage image;
    DevBuf keep, red, counts, total, kept, kA, kB, vA, vB, kind, full_heads, open_heads, heads, lengths, centres, table, open_lengths,
        rows, order;
    RadixScratch scratch;
};

// the positions j < n with kind[j] == match -> out (allocated here), their number -> *found.  Synchronises.
int compact(EncodeBuffers& B, const uint8_t* kind, uint32_t match, uint32_t n, DevBuf& out, uint32_t* found, hipStream_t st) {
    const uint32_t blocks = grid_of(n);
    GS_TRY(B.counts.ensure(sizeof(uint32_t) * blocks));
    hipLaunchKernelGGL(k_cmp_count, dim3(blocks), dim3(256), 0, st, kind, match, n, B.counts.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, st, B.counts.as<uint32_t>(), blocks, B.total.as<uint32_t>());
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(found, B.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    if (*found == 0) return GS_OK;
    GS_TRY(out.ensure(sizeof(uint32_t) * (size_t)*found));
    hipLaunchKernelGGL(k_cmp_write, dim3(blocks), dim3(256), 0, st, kind, match, n, B.counts.as<uint32_t>(), out.as<uint32_t>());
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// stable sort of (keys, vals) in kA / vA by all 32 key bits: four passes, so the result is in kA / vA again
int sort_pairs(gs_context* ctx, EncodeBuffers& B, uint32_t n, hipStream_t st) {
    GS_HIP(hipMemsetAsync(B.scratch.digit_total.p, 0, sizeof(uint32_t) * RADIX_TOTAL_WORDS, st));
    uint32_t* kbuf[2] = {B.kA.as<uint32_t>(), B.kB.as<uint32_t>()};
    uint32_t* vbuf[2] = {B.vA.as<uint32_t>(), B.vB.as<uint32_t>()};
    const RadixExec ex = {st, &B.scratch, ctx->lds_atomic_lane_order};
    for (int pass = 0; pass < 4; pass++) {
        ArrayLoader<uint32_t> al = {kbuf[pass & 1], vbuf[pass & 1], nullptr, n};
        GS_TRY((radix_pass<ArrayLoader<uint32_t>, uint32_t, true>(ex, al, al, n, 8 * pass, pass, kbuf[(pass + 1) & 1], vbuf[(pass + 1) & 1])));
    }
    return GS_OK;
}

// The range rule as the reference runs it (:1193-1205), for the side the device found no value of its sign for: the host's
// level-0 rows, every row in file order.  lower: the minimum (`<`), else the maximum (`>`).
double sh_bound_sequential(const gs_asset* a, uint32_t nscan, bool lower) {
    const KsplatSource img = a->image();
    bool has = false;
    double m = 0.0;
    for (uint32_t i = 0; i < a->splat_count; i++) {
        const auto row = img.row(i);
        for (uint32_t s = 0; s < nscan; s++) {
            const double val = row.sh_wide(s, 0.0, 0.0);
            if (!has || m == 0.0 || m != m || (lower ? val < m : val > m)) {
                m = val;
                has = true;
            }
        }
    }
    return (has && m == m && m != 0.0) ? m : (lower ? -1.5 : 1.5);
}

struct Resolved {
    uint32_t level, min_alpha, bucket_size;
    double block;
    float scene_center[3];
};

template <class Source>
int encode(gs_context* ctx, gs_asset* a, const Resolved& p, std::vector<uint8_t>& file, uint32_t* order_out_host) {
#pragma clang fp contract(off)
    hipStream_t st = ctx->stream;
    EncodeBuffers B;
    const uint32_t n = a->splat_count, ncomp = sh_components(a->sh_degree), nscan = ncomp < 23u ? ncomp : 23u;
    Source src;
    GS_TRY(asset_stage(a, 0, n, B.image, st, &src, false));
    GS_TRY(B.scratch.init());
    GS_TRY(B.keep.alloc(n));
    GS_TRY(B.red.alloc(sizeof(uint32_t) * RED_WORDS));
    GS_TRY(B.total.alloc(sizeof(uint32_t)));
    uint32_t red[RED_WORDS];
    for (uint32_t k = 0; k < RED_WORDS; k++) red[k] = k < RED_MAX ? 0xFFFFFFFFu : 0u;
    GS_HIP(hipMemcpyAsync(B.red.p, red, sizeof(red), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_enc_flags<Source>), dim3(grid_of(n)), dim3(256), 0, st, src, n, p.min_alpha, nscan, B.keep.as<uint8_t>(), B.red.as<uint32_t>());
    GS_HIP(hipGetLastError());
    uint32_t count = 0;
    GS_TRY(compact(B, B.keep.as<uint8_t>(), 1u, n, B.kept, &count, st));
    GS_HIP(hipMemcpyAsync(red, B.red.p, sizeof(red), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    GS_REQUIRE(count > 0, "no splat survives min_alpha");
    GS_REQUIRE(red[RED_BAD] == 0, "a kept centre is not finite");

    EncParams P = {};
    double mx[3], blocks[3], top[3];
    for (int k = 0; k < 3; k++) {
        P.mn[k] = (double)ordered_float(red[RED_MIN + k]);
        mx[k] = (double)ordered_float(red[RED_MAX + k]);
        blocks[k] = ceil((mx[k] - P.mn[k]) / p.block);         // x/y/zBlocks (:1348-1350; x's is not used by the reference)
        top[k] = floor((mx[k] - P.mn[k]) / p.block);           // the greatest block index along the axis
    }
    P.block = p.block;
    P.half_block = p.block / 2.0;
    P.yz_blocks = blocks[1] * blocks[2];
    P.z_blocks = blocks[2];
    P.scale_factor = 32767.0 / (p.block * 0.5);
    P.level = p.level;
    P.ncomp = ncomp;
    P.bucket_size = p.bucket_size;
    const double greatest_id = top[0] * P.yz_blocks + top[1] * P.z_blocks + top[2];
    if (!((blocks[0] + 1.0) * P.yz_blocks < 4294967295.0) || !(greatest_id < 4294967295.0)) {
        gs_set_error("unsupported: the scene spans 2^32 - 1 or more blocks of block_size: bucket ids stop being array indexes");
        return GS_ERR_UNSUPPORTED;
    }
    P.sh_lo = -1.5;
    P.sh_hi = 1.5;
    if (nscan) {
        if (!red[RED_SH_NEG] || !red[RED_SH_POS])               // the whole scan is the sequential prefix: the host's rows
            GS_TRY(gs_asset_fill(a, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        P.sh_lo = red[RED_SH_NEG] ? (double)__builtin_bit_cast(float, red[RED_SH_NEG]) : sh_bound_sequential(a, nscan, true);
        P.sh_hi = red[RED_SH_POS] ? (double)__builtin_bit_cast(float, red[RED_SH_POS]) : sh_bound_sequential(a, nscan, false);
    }

    // cells, the stable sort by cell, the bucket heads
    const size_t words = sizeof(uint32_t) * (size_t)count;
    GS_TRY(B.kA.alloc(words)); GS_TRY(B.kB.alloc(words)); GS_TRY(B.vA.alloc(words)); GS_TRY(B.vB.alloc(words));
    GS_TRY(B.kind.alloc(count));
    hipLaunchKernelGGL((k_enc_cells<Source>), dim3(grid_of(count)), dim3(256), 0, st, src, P, B.kept.as<uint32_t>(), count,
                       B.kA.as<uint32_t>(), B.vA.as<uint32_t>());
    GS_HIP(hipGetLastError());
    GS_TRY(sort_pairs(ctx, B, count, st));
    hipLaunchKernelGGL(k_enc_heads, dim3(grid_of(count)), dim3(256), 0, st, B.kA.as<uint32_t>(), count, p.bucket_size, B.kind.as<uint8_t>());
    GS_HIP(hipGetLastError());
    uint32_t full = 0, open = 0;
    GS_TRY(compact(B, B.kind.as<uint8_t>(), HEAD_FULL, count, B.full_heads, &full, st));
    GS_TRY(compact(B, B.kind.as<uint8_t>(), HEAD_OPEN, count, B.open_heads, &open, st));
    const uint32_t buckets = full + open;                      // >= 1: count > 0
    // the sorted cells are needed below and the second sort runs in the same four buffers: keep them aside
    DevBuf cell_keys, cell_vals;
    GS_TRY(B.heads.alloc(sizeof(uint32_t) * (size_t)buckets));
    if (full) {
        GS_TRY(cell_keys.alloc(words)); GS_TRY(cell_vals.alloc(words));
        GS_HIP(hipMemcpyAsync(cell_keys.p, B.kA.p, words, hipMemcpyDeviceToDevice, st));
        GS_HIP(hipMemcpyAsync(cell_vals.p, B.vA.p, words, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_enc_close_keys, dim3(grid_of(full)), dim3(256), 0, st, B.full_heads.as<uint32_t>(), full, cell_vals.as<uint32_t>(),
                           p.bucket_size, B.kA.as<uint32_t>(), B.vA.as<uint32_t>());
        GS_HIP(hipGetLastError());
        GS_TRY(sort_pairs(ctx, B, full, st));
        GS_HIP(hipMemcpyAsync(B.heads.p, B.vA.p, sizeof(uint32_t) * (size_t)full, hipMemcpyDeviceToDevice, st));
    }
    const uint32_t* sorted_keys = full ? cell_keys.as<uint32_t>() : B.kA.as<uint32_t>();
    const uint32_t* sorted_vals = full ? cell_vals.as<uint32_t>() : B.vA.as<uint32_t>();
    if (open)
        GS_HIP(hipMemcpyAsync(B.heads.as<uint32_t>() + full, B.open_heads.p, sizeof(uint32_t) * (size_t)open, hipMemcpyDeviceToDevice, st));

    gs_ksplat_layout lay;
    ksplat_layout(p.level, a->sh_degree, count, full, open, &lay);
    if (lay.storage_bytes > 0xFFFFFFFFull) {
        gs_set_error("unsupported: the section would exceed the 4 GiB its header can state");
        return GS_ERR_UNSUPPORTED;
    }
    P.bytes_per_splat = lay.bytes_per_splat;
    const size_t row_bytes = (size_t)lay.bytes_per_splat * count;
    GS_TRY(B.lengths.alloc(sizeof(uint32_t) * (size_t)buckets));
    GS_TRY(B.centres.alloc(sizeof(double) * 3 * (size_t)buckets));
    GS_TRY(B.table.alloc(sizeof(float) * 3 * (size_t)buckets));
    GS_TRY(B.open_lengths.alloc(sizeof(uint32_t) * (size_t)(open ? open : 1u)));
    GS_TRY(B.rows.alloc((row_bytes + 3) & ~(size_t)3));
    GS_TRY(B.order.alloc(words));
    hipLaunchKernelGGL((k_enc_buckets<Source>), dim3(grid_of(buckets)), dim3(256), 0, st, src, P, B.kept.as<uint32_t>(), sorted_keys, sorted_vals, count,
                       B.heads.as<uint32_t>(), buckets, full, B.lengths.as<uint32_t>(), B.centres.as<double>(), B.table.as<float>(),
                       B.open_lengths.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, st, B.lengths.as<uint32_t>(), buckets, B.total.as<uint32_t>());
    hipLaunchKernelGGL((k_enc_rows<Source>), dim3(grid_of(count)), dim3(256), 0, st, src, P, B.kept.as<uint32_t>(), sorted_vals, B.heads.as<uint32_t>(),
                       B.lengths.as<uint32_t>(), buckets, B.centres.as<double>(), count, B.rows.as<uint8_t>(), B.order.as<uint32_t>());
    GS_HIP(hipGetLastError());

    // the file: writeHeaderToBuffer :856-875, writeSectionHeaderToBuffer :944-960, the section :1260-1274
    file.assign((size_t)lay.total_bytes, 0);
    uint8_t* F = file.data();
    auto W32 = [&](size_t off, uint32_t v) { memcpy(F + off, &v, 4); };
    auto W16 = [&](size_t off, uint16_t v) { memcpy(F + off, &v, 2); };
    auto WF = [&](size_t off, float v) { memcpy(F + off, &v, 4); };
    F[0] = 0; F[1] = 1;
    W32(4, 1); W32(8, 1); W32(12, count); W32(16, count); W16(20, (uint16_t)p.level);
    for (int k = 0; k < 3; k++) WF(24 + 4 * k, p.scene_center[k]);
    WF(36, (float)P.sh_lo); WF(40, (float)P.sh_hi);
    const size_t h = 4096;
    W32(h + 0, count); W32(h + 4, count);
    if (p.level >= 1) {
        W32(h + 8, p.bucket_size); W32(h + 12, buckets); WF(h + 16, (float)p.block); W16(h + 20, 12); W32(h + 24, 32767u);
        W32(h + 32, full); W32(h + 36, open);
    }
    W32(h + 28, (uint32_t)lay.storage_bytes);
    W16(h + 40, (uint16_t)a->sh_degree);
    if (p.level >= 1) {
        if (open) GS_HIP(hipMemcpyAsync(F + lay.partial_off, B.open_lengths.p, 4 * (size_t)open, hipMemcpyDeviceToHost, st));
        GS_HIP(hipMemcpyAsync(F + lay.buckets_off, B.table.p, 12 * (size_t)buckets, hipMemcpyDeviceToHost, st));
    }
    GS_HIP(hipMemcpyAsync(F + lay.rows_off, B.rows.p, row_bytes, hipMemcpyDeviceToHost, st));
    if (order_out_host) GS_HIP(hipMemcpyAsync(order_out_host, B.order.p, words, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_asset_encode_ksplat(gs_context* ctx, gs_asset* src, const gs_ksplat_params* params, gs_asset** out, uint32_t* order_out_host) {
    GS_REQUIRE(src && params && out, "asset / params / out == NULL");
    *out = nullptr;
    Resolved p;
    p.level = params->compression_level;
    p.min_alpha = params->min_alpha;
    p.bucket_size = params->bucket_size ? params->bucket_size : 256u;        // `bucketSize || SplatBuffer.BucketSize` :1226
    p.block = params->block_size != 0.0f ? (double)params->block_size : 5.0;   // `blockSize || SplatBuffer.BucketBlockSize` :1225
    for (int k = 0; k < 3; k++) p.scene_center[k] = params->scene_center[k];
    GS_REQUIRE(p.level <= 2, "compression_level outside 0..2");
    GS_REQUIRE(params->flags == 0, "unknown flags");
    GS_REQUIRE(p.block == p.block && p.block > 0.0 && p.block < (double)INFINITY, "block_size is not a finite number above 0");
    GS_REQUIRE(p.bucket_size <= 65535u, "bucket_size above 65535");
    GS_REQUIRE(!src->incomplete(), "the source is a stream that is not complete");
    if (src->level != 0) {
        gs_set_error("unsupported: the source is a compression level %u .ksplat: its values are quantised already", src->level);
        return GS_ERR_UNSUPPORTED;
    }
    GS_REQUIRE(!src->has_transform, "the source has a scene transform (gs_asset_set_transform(a, NULL) removes it)");
    GS_REQUIRE(src->splat_count > 0, "no splat survives min_alpha: the source has none");
    GS_REQUIRE(ctx != nullptr, "context == NULL");
    ScopedDevice sd(ctx->device);
    std::vector<uint8_t> file;
    try {
        GS_TRY(with_source_of(src, [&](auto source) { return encode<typename decltype(source)::type>(ctx, src, p, file, order_out_host); }));
    } catch (const std::bad_alloc&) {
        gs_set_error("out of host memory while encoding the asset");
        return GS_ERR_NOMEM;
    }
    gs_asset* made = nullptr;
    GS_TRY(gs_asset_open(file.data(), file.size(), GS_ASSET_KSPLAT, 2, &made));
    made->encoded = true;
    *out = made;
    return GS_OK;
}

int gs_asset_bytes(gs_asset* a, const void** data, uint64_t* bytes) {
    GS_REQUIRE(a && data && bytes, "asset / data / bytes == NULL");
    GS_REQUIRE(a->encoded, "the asset is no result of gs_asset_encode_ksplat");
    *data = a->buf.data();
    *bytes = a->buf.size();
    return GS_OK;
}

}  // extern "C"
