// asset_sources.hpp — the device row sources of an opened asset and the staging of a range of its rows: what the decode
// kernels (asset_decode.hip) and the .ksplat encoder (asset_encode.hip) both template on.  A source says where splat i's values
// come from (the Row interface: asset_internal.hpp); asset_stage uploads what a source reads of a range and hands the source back.
#pragma once
#include <algorithm>

#include "asset_internal.hpp"

namespace {

// ---- row sources over file rows (the Row interface: asset_internal.hpp) ------------------------------------------------------------
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

// INRIA-v2 codebook PLY: the file's rows at their own stride (17 / 26 / 41 / 62 bytes and whatever extra properties add), row 0 at the
// staging base.  A row is one index byte per attribute and three centre halves at any byte phase, so it is read with byte loads
// (neighbouring lanes meet in the same cache lines): no load reaches past the row, let alone into the padding behind the last one.
// The decoded codebook (assets.hip decodes it at open) is a table of 256-float pages; k_asset_decode copies the pages its degree
// reads into LDS first (load_table), since a splat makes up to 38 data-dependent look-ups into them; k_asset_centers reads none.
struct InriaV2Source {
    const uint8_t* rows;           // row 0 = asset splat `base`
    const float* codebook;         // the decoded table: global memory (16-byte aligned) until load_table puts its LDS copy here
    uint32_t base;
    uint32_t level, sh_degree, ncomp;   // 0, the output degree, 0 / 9 / 24
    InriaV2Layout layout;
    struct Row : TupleValues {
        const uint8_t* row;
        const InriaV2Layout& L;
        const float* codebook;
        __device__ __forceinline__ float value(uint32_t src) const { return inria_v2_row_sh(row, L, codebook, src); }
        __device__ __forceinline__ double sh_wide(uint32_t src, double, double) const { return (double)value(src); }
        __device__ __forceinline__ uint16_t sh_half(uint32_t src) const { return to_half_three((double)value(src)); }
        __device__ __forceinline__ uint8_t sh_byte(uint32_t) const { return 0; }   // sh_level is 1: never stored as bytes
    };
    __device__ __forceinline__ const uint8_t* row_of(uint32_t splat) const { return rows + (size_t)layout.stride * (splat - base); }
    __device__ __forceinline__ Row row(uint32_t splat) const {
        Row r = {{}, row_of(splat), layout, codebook};
        inria_v2_row_tuple(r.row, layout, codebook, r.t);
        return r;
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const {    // the three halves alone
        float c[3];
        inria_v2_row_centre(row_of(splat), layout, c);
        for (int k = 0; k < 3; k++) d[k] = c[k];
    }
    // Every thread of the workgroup, the ones past the range's end too: the pages the output degree reads (a prefix of the table),
    // as coalesced 16-byte loads, then the barrier.
    __device__ __forceinline__ void load_table(float* lds) {
        const uint32_t quads = 64u * inria_v2_pages_read(sh_degree);
        for (uint32_t k = threadIdx.x; k < quads; k += 256u) reinterpret_cast<float4*>(lds)[k] = reinterpret_cast<const float4*>(codebook)[k];
        __syncthreads();
        codebook = lds;
    }
};

// A streamed INRIA-v1 PLY: the trainer's own rows at their file stride (68 bytes at degree 0, 248 at degree 3, odd with a uchar
// property), row 0 at the staging base - the header has any length, so nothing else is known of a row's alignment.  A thread reads
// its row's fields in place: when the stride and every 4-byte field's offset are multiples of 4 (layout.aligned: every file of
// floats), each is one aligned dword load, else it is put together from byte loads; no load reaches past the row.  Neighbouring
// lanes are a stride apart, so a wave's loads of one field touch 64 rows' cache lines, and the lines are used up as the thread walks
// its fields.  k_asset_centers reads x, y and z alone.
struct InriaV1Source {
    const uint8_t* rows;           // row 0 = asset splat `base`
    uint32_t base;
    uint32_t level, sh_degree, ncomp;   // 0, the output degree, 0 / 9 / 24
    InriaV1Layout layout;
    struct Row : TupleValues {
        const uint8_t* row;
        const InriaV1Layout& L;
        bool has_sh;               // the row has an f_rest_0: read once, not per SH slot
        __device__ __forceinline__ float value(uint32_t src) const { return inria_v1_row_sh(row, L, has_sh, src); }
        __device__ __forceinline__ double sh_wide(uint32_t src, double, double) const { return (double)value(src); }
        __device__ __forceinline__ uint16_t sh_half(uint32_t src) const { return to_half_three((double)value(src)); }
        __device__ __forceinline__ uint8_t sh_byte(uint32_t) const { return 0; }   // sh_level is 1: never stored as bytes
    };
    __device__ __forceinline__ const uint8_t* row_of(uint32_t splat) const { return rows + (size_t)layout.stride * (splat - base); }
    __device__ __forceinline__ Row row(uint32_t splat) const {
        Row r = {{}, row_of(splat), layout, false};
        r.has_sh = ncomp != 0 && inria_v1_row_has_sh(r.row, layout);
        inria_v1_row_tuple(r.row, layout, r.t);
        return r;
    }
    __device__ __forceinline__ void centre(uint32_t splat, double d[3]) const {    // x, y, z alone
        float c[3];
        inria_v1_row_centre(row_of(splat), layout, c);
        for (int k = 0; k < 3; k++) d[k] = c[k];
    }
};

// floats of LDS a source's workgroup fills before its threads decode (Source::load_table): the 13 pages degree 2 reads
template <class Source> struct LdsTable { static constexpr uint32_t floats = 0; };
template <> struct LdsTable<InriaV2Source> { static constexpr uint32_t floats = 256u * (IV2_PAGE_REST + 8u); };

// Uploads what the kernels read of splats [first, first + count), count > 0, in range: their rows (one contiguous piece of the
// file), the bucket tables of their sections and the section records, rebased onto the staged pieces.  Synchronises `st`: the
// host table is a local.  centres_only (every asset_stage): the sorter's message reads centres alone, so a source that keeps other
// values apart from them leaves those at home; a .ksplat row (and a .splat row) holds the centre among the rest.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, KsplatSource* view, bool centres_only) {
    (void)centres_only;
    GS_REQUIRE(!a->sections.empty(), "the asset has no section for the range");
    const KsplatSource file = a->image();
    const uint32_t last = first + count - 1u;
    const KsplatSection &sa = section_of(file, first), &sb = section_of(file, last);
    const size_t lo = (size_t)sa.data_off + (size_t)sa.bytes_per_splat * (first - sa.count_offset);
    const size_t hi = (size_t)sb.data_off + (size_t)sb.bytes_per_splat * (last - sb.count_offset + 1u);
    const uint32_t partial_lo = sa.partial_begin, partial_hi = sb.partial_begin + sb.partial_count;
    std::vector<KsplatSection> table(&sa, &sb + 1);
    size_t bytes = (hi - lo + 15) & ~(size_t)15;
    for (KsplatSection& d : table) {
        d.data_off -= (long long)lo;
        d.partial_begin -= partial_lo;
        d.buckets_off = (long long)bytes;
        if (a->level > 0) bytes += ((size_t)d.bucket_storage * d.bucket_count + 15) & ~(size_t)15;   // only read for compressed centres
    }
    const size_t table_bytes = table.size() * sizeof(KsplatSection), partial_bytes = (size_t)(partial_hi - partial_lo) * 4;
    GS_TRY(dev.bytes.ensure(bytes));
    GS_TRY(dev.table.ensure(table_bytes + partial_bytes + 16));
    uint8_t* image = dev.bytes.as<uint8_t>();
    GS_HIP(hipMemcpyAsync(image, file.image + lo, hi - lo, hipMemcpyHostToDevice, st));
    if (a->level > 0)
        for (size_t k = 0; k < table.size(); k++)
            if (table[k].bucket_count)
                GS_HIP(hipMemcpyAsync(image + table[k].buckets_off, file.image + (&sa)[k].buckets_off,
                                      (size_t)table[k].bucket_storage * table[k].bucket_count, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(dev.table.p, table.data(), table_bytes, hipMemcpyHostToDevice, st));
    if (partial_bytes)
        GS_HIP(hipMemcpyAsync(dev.table.as<char>() + table_bytes, file.partial_end + partial_lo, partial_bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    *view = file;
    view->image = image;
    view->sections = dev.table.as<KsplatSection>();
    view->partial_end = reinterpret_cast<const uint32_t*>(dev.table.as<char>() + table_bytes);
    view->section_count = (uint32_t)table.size();
    return GS_OK;
}

// .splat: rows [first, first + count) at the staging base
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, SplatSource* src, bool centres_only) {
    (void)centres_only;
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

// INRIA-v2 PLY: rows [first, first + count) at their file stride, one piece at the staging base, padded to 16 bytes, and - unless only
// centres are wanted (they lie in the row) - the decoded codebook (20 KiB).  gs_asset_open proved that the file holds every row.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, InriaV2Source* src, bool centres_only) {
    const size_t stride = a->iv2.stride, bytes = stride * count, table_bytes = a->iv2_codebook.size() * sizeof(float);
    GS_TRY(dev.bytes.ensure((bytes + 15) & ~(size_t)15));
    GS_HIP(hipMemcpyAsync(dev.bytes.p, a->file.data() + a->iv2_vertex_base + stride * first, bytes, hipMemcpyHostToDevice, st));
    if (!centres_only) {
        GS_TRY(dev.table.ensure(table_bytes));
        GS_HIP(hipMemcpyAsync(dev.table.p, a->iv2_codebook.data(), table_bytes, hipMemcpyHostToDevice, st));
    }
    GS_HIP(hipStreamSynchronize(st));
    *src = InriaV2Source{dev.bytes.as<uint8_t>(), centres_only ? nullptr : dev.table.as<float>(), first, 0u, a->sh_degree,
                         sh_components(a->sh_degree), a->iv2};
    return GS_OK;
}

// A streamed INRIA-v1 PLY: rows [first, first + count) at their file stride, one piece at the staging base, padded to 16 bytes.  The
// caller proved the range ready: every byte of these rows has arrived.
int asset_stage(const gs_asset* a, uint32_t first, uint32_t count, AssetDeviceImage& dev, hipStream_t st, InriaV1Source* src, bool centres_only) {
    (void)centres_only;                                      // the centre lies in the row
    const size_t stride = a->iv1.stride, bytes = stride * count;
    GS_TRY(dev.bytes.ensure(((bytes + 15) & ~(size_t)15) + 16));
    if (bytes) GS_HIP(hipMemcpyAsync(dev.bytes.p, a->file.data() + a->iv1_vertex_base + stride * first, bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipStreamSynchronize(st));
    *src = InriaV1Source{dev.bytes.as<uint8_t>(), first, 0u, a->sh_degree, sh_components(a->sh_degree), a->iv1};
    return GS_OK;
}

// a->rows -> the source type of its rows: f(SourceOf<Source>())
template <class Source>
struct SourceOf { using type = Source; };
template <class F>
int with_source_of(const gs_asset* a, F f) {
    switch (a->rows) {
        case ASSET_ROWS_SPLAT: return f(SourceOf<SplatSource>());
        case ASSET_ROWS_COMPRESSED_PLY: return f(SourceOf<CompressedSource>());
        case ASSET_ROWS_SPZ: return f(SourceOf<SpzSource>());
        case ASSET_ROWS_INRIA_V2: return f(SourceOf<InriaV2Source>());
        case ASSET_ROWS_INRIA_V1: return f(SourceOf<InriaV1Source>());
        default: return f(SourceOf<KsplatSource>());
    }
}

}  // namespace
