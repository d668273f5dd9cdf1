// assets.hip — native asset readers (host code; asset_decode.hip decodes the same image per splat on the device, through the
// same .ksplat row reader and per-splat fill body: asset_internal.hpp says both once for the two sides): INRIA-v1 .ply,
// PlayCanvas compressed .ply, INRIA-v2 codebook .ply, .splat, .spz and .ksplat -> the arrays the render / sort seams consume.
// Restates, never copies:
//   INRIA-v2 PLY      src/loaders/ply/INRIAV2PlyParser.js:45-126 (sections), :128-160 (decodeCodeBook: decoded once, at open, with
//                     every per-row rule that depends on the entry alone, so an entry is one fp32); the row arithmetic (:202-269 +
//                     SplatBuffer.js:1092-1124) is in asset_internal.hpp, shared with the device.  FILE ORDER, as .splat below: the
//                     reference has no file-order path for it (PlyParser.parseToUncompressedSplatBuffer throws), and its array path
//                     drops and reorders; splat i here is the level-0 row of parseToUncompressedSplat(file row i)
//   .spz              src/loaders/spz/SpzLoader.js:255-342 (container; the gzip reader and every refusal are in spz_container.hpp),
//                     :366-388 with optimizeSplatData false (file order); the row arithmetic (:160-250, 84-145 + SplatBuffer.js
//                     :1092-1124) is in asset_internal.hpp, shared with the device
//   PLY flavour       src/loaders/ply/PlyParserUtils.js:257-271 (determineHeaderFormatFromHeaderText)
//   compressed PLY    src/loaders/ply/PlayCanvasCompressedPlyParser.js:74-157 (decodeHeaderText), :159-242 (decodeHeader); the row
//                     arithmetic (:379-460 + SplatBuffer.js:1092-1124) is in asset_internal.hpp, shared with the device
//   .splat            src/loaders/splat/SplatParser.js:13-56 (parseToUncompressedSplatBufferSection): the reference's
//                     progressive, FILE-ORDER path - every splat is kept, alpha is only zeroed at fill time by min_alpha.  The
//                     `optimizeSplatData: false` array path (SplatLoader.js:12-22) drops splats below minimumAlpha and reorders
//                     them bucket by bucket; that is not what "file order" means here and is not restated.
//   PLY header        src/loaders/ply/PlyParserUtils.js:31-165 (decodeSectionHeader, SH field mapping),
//                     INRIAV1PlyParser.js:20-47 (fields read)
//   PLY row -> splat  INRIAV1PlyParser.js:114-209 (exp scale, sigmoid opacity, floor/clamp colours, quaternion normalise)
//                     + SplatBuffer.writeSplatDataToSectionBuffer :1056-1113 (level-0 row: second normalise, fp32 stores)
//   .ksplat layout    SplatBuffer.js:819-848 (header), :877-941 (section headers); rows per compression level, the bucket of a
//                     splat and the centre decode are in asset_internal.hpp
//   arrays            asset_fill_splat (asset_internal.hpp) for every splat of the image; which outputs a call may ask for:
//                     SH target level = max(1, buffer level) (SplatMesh.js:1064-1066); WITHOUT a scene
//                     transform (dynamicMode) until gs_asset_set_transform gives one (static mode, SplatMesh.js:1872-1899):
//                     then Vector3.applyMatrix4 :340-342, T3*C*T3^T :461-466, rotated SH :628-637, 684-688, 707-715, 766-817
//   scene transform   three r160 Matrix4.decompose / Quaternion.setFromRotationMatrix / normalize / makeRotationFromQuaternion
// An INRIA-v1 PLY is first laid out as the level-0 section the reference would build from it (file order, i.e. the reference's
// `optimizeSplatData: false`), so every fill routine reads one format.  A .splat / compressed PLY / INRIA-v2 PLY / .spz asset keeps
// the file's own rows (for .spz: the inflated planes; what the device decode uploads) and builds that level-0 section when a host
// fill first needs it.
// Reference quirk, documented and not reproduced: PlayCanvasCompressedPlyParser.readPly (:297-313) throws on a compressed PLY
// without an `sh` element (TypeError: 'count' of undefined); the progressive path loads such files, and so does this reader.
// INRIAV2PlyParser.parseToUncompressedSplat keeps its raw row in a closure across calls, so a file that lacks a field can see the
// previous file's last row; this reader behaves as a fresh parser does (absent scale_* -> 0.01, absent f_dc_* / opacity -> 0).
#include <algorithm>
#include <math.h>
#include <string>

#include "asset_internal.hpp"

namespace {

uint8_t clamped_u8(double v) {                         // Uint8ClampedArray store: NaN -> 0, round half to even
    if (!(v == v)) return 0;
    if (v <= 0.0) return 0;
    if (v >= 255.0) return 255;
    return (uint8_t)nearbyint(v);
}

constexpr size_t KS_HEADER = 4096, KS_SECTION_HEADER = 1024;

// whole: `buf` is the file, and what does not fit into it is refused.  Else `buf` is the prefix of a stream (gs_asset_append): what
// has not arrived is waited for (STREAM_NEED_MORE before the header and every section header are in), `sections` receives the
// sections whose bucket block has arrived and passed the table checks - in file order, stopping at the first that has not - and
// `runs` says from which byte on their rows are ready.
const char KS_DATA_EXCEEDS[] = ".ksplat: section data exceeds the file";
int parse_ksplat(gs_asset* a, bool whole = true, std::vector<StreamRun>* runs = nullptr, size_t* file_end = nullptr) {
    const size_t n = a->buf.size();
    if (!whole && n < KS_HEADER) return STREAM_NEED_MORE;
    GS_REQUIRE(n >= KS_HEADER, ".ksplat: shorter than its 4096-byte header");
    const uint32_t max_sections = a->rd<uint32_t>(4), max_splats = a->rd<uint32_t>(12);
    a->level = a->rd<uint16_t>(20);
    GS_REQUIRE(a->level <= 2, ".ksplat: unknown compression level");
    for (int k = 0; k < 3; k++) a->scene_center[k] = a->rd<float>(24 + 4 * k);
    const float mn = a->rd<float>(36), mx = a->rd<float>(40);
    a->sh_min = mn != 0.0f ? (double)mn : -1.5;            // `|| -DefaultSphericalHarmonics8BitCompressionHalfRange`
    a->sh_max = mx != 0.0f ? (double)mx : 1.5;
    if (!whole && KS_HEADER + (size_t)max_sections * KS_SECTION_HEADER > n) return STREAM_NEED_MORE;
    GS_REQUIRE(KS_HEADER + (size_t)max_sections * KS_SECTION_HEADER <= n, ".ksplat: section headers exceed the file");
    bool arrived = true;                                    // (a stream) every bucket block so far is in
    size_t base = KS_HEADER + (size_t)max_sections * KS_SECTION_HEADER;
    uint32_t count_offset = 0;
    uint32_t min_degree = 0;
    a->sections.clear();
    a->partial_end.clear();
    for (uint32_t s = 0; s < max_sections; s++) {
        const size_t h = KS_HEADER + (size_t)s * KS_SECTION_HEADER;
        KsplatSection sec = {};
        sec.count = a->rd<uint32_t>(h + 4);                // maxSplatCount: secLoadedCountsToMax
        sec.bucket_size = a->rd<uint32_t>(h + 8);
        sec.bucket_count = a->rd<uint32_t>(h + 12);
        const double half_block = (double)a->rd<float>(h + 16) / 2.0;
        sec.bucket_storage = a->rd<uint16_t>(h + 20);
        const uint32_t range = a->rd<uint32_t>(h + 24);
        sec.scale_range = range ? range : (a->level == 0 ? 1u : 32767u);
        sec.scale_factor = half_block / (double)sec.scale_range;
        sec.full_buckets = a->rd<uint32_t>(h + 32);
        const uint32_t partial_buckets = a->rd<uint32_t>(h + 36), sh_degree = a->rd<uint16_t>(h + 40);
        GS_REQUIRE(sh_degree <= 2, ".ksplat: spherical harmonics degree > 2");
        sec.bytes_per_splat = asset_center_bytes(a->level) + asset_scale_bytes(a->level) + asset_rotation_bytes(a->level) + 4u +
                              asset_sh_value_bytes(a->level) * sh_components(sh_degree);
        const size_t meta = (size_t)partial_buckets * 4, buckets = (size_t)sec.bucket_storage * sec.bucket_count + meta;
        sec.buckets_off = (long long)(base + meta);
        sec.data_off = (long long)(base + buckets);
        sec.count_offset = count_offset;
        const size_t end = base + buckets + (size_t)sec.bytes_per_splat * sec.count;
        GS_REQUIRE(!whole || end <= n, KS_DATA_EXCEEDS);
        arrived = arrived && base + buckets <= n;
        sec.partial_begin = (uint32_t)a->partial_end.size();
        if (arrived && a->level > 0 && sec.count > 0) {
            // Bucket tables are only read for compressed centres (SplatBuffer.js:199-246).  The reference is memory-safe
            // JavaScript; here every index into the tables is proven in range before a row read goes through them.
            GS_REQUIRE(sec.bucket_storage >= 12, ".ksplat: bucket storage below the 12 bytes of a bucket centre");
            GS_REQUIRE(sec.bucket_size > 0, ".ksplat: bucket size 0 in a compressed section");
            GS_REQUIRE((uint64_t)sec.full_buckets + partial_buckets <= sec.bucket_count,
                       ".ksplat: more full + partial buckets than the section stores");
            uint64_t covered = (uint64_t)sec.full_buckets * sec.bucket_size;
            GS_REQUIRE(covered <= 0xFFFFFFFFull, ".ksplat: full buckets x bucket size overflows 32 bits");   // bucket_index's span
            for (uint32_t p = 0; p < partial_buckets; p++) {
                covered += a->rd<uint32_t>(base + 4 * (size_t)p);
                GS_REQUIRE(covered <= 0xFFFFFFFFull, ".ksplat: partial bucket lengths overflow");
                a->partial_end.push_back((uint32_t)covered);
            }
            GS_REQUIRE(covered >= sec.count, ".ksplat: the buckets do not cover every splat of the section");
            sec.partial_count = partial_buckets;
        }
        base = end;
        count_offset += sec.count;
        if (s == 0 || sh_degree < min_degree) min_degree = sh_degree;   // getMinSphericalHarmonicsDegree
        if (sec.count > 0 && arrived) {
            a->sections.push_back(sec);                     // section_of looks among the ones that hold splats
            if (runs) runs->push_back({(uint64_t)sec.data_off, (uint64_t)sec.data_off, sec.bytes_per_splat, sec.count_offset, sec.count});
        }
    }
    GS_REQUIRE(count_offset == max_splats || max_sections == 0 || count_offset >= max_splats, ".ksplat: splat counts disagree");
    a->splat_count = count_offset < max_splats ? count_offset : max_splats;
    a->sh_degree = min_degree;
    if (file_end) *file_end = base;
    return GS_OK;
}

// ---- the level-0 image an INRIA-v1 PLY and the row formats are laid out as ------------------------------
// SplatBuffer.preallocateUncompressed (:1401-1433): header + one section header, rows of 44 + 4 * ncomp bytes
void level0_header(std::vector<uint8_t>& buf, uint32_t count, uint32_t degree) {
    const uint32_t bps = 44u + 4u * sh_components(degree);
    buf.assign(KS_HEADER + KS_SECTION_HEADER + (size_t)bps * count, 0);
    uint8_t* B = buf.data();
    auto W32 = [&](size_t off, uint32_t v) { memcpy(B + off, &v, 4); };
    auto W16 = [&](size_t off, uint16_t v) { memcpy(B + off, &v, 2); };
    auto WF = [&](size_t off, float v) { memcpy(B + off, &v, 4); };
    B[0] = 0; B[1] = 1;
    W32(4, 1); W32(8, 1); W32(12, count); W32(16, count); W16(20, 0);
    WF(36, -1.5f); WF(40, 1.5f);
    W32(KS_HEADER + 0, count); W32(KS_HEADER + 4, count); W16(KS_HEADER + 40, (uint16_t)degree);
}
void store_level0_row(uint8_t* o, const Level0Tuple& t) {
    memcpy(o, t.c, 12); memcpy(o + 12, t.s, 12); memcpy(o + 24, t.r, 16); memcpy(o + 40, t.rgba, 4);
}
void store_level0_sh(uint8_t* o, uint32_t s, float v) { memcpy(o + 44 + 4 * s, &v, 4); }   // SH float s of the row

// ---- PLY ------------------------------------------------------------------------------------------
enum FieldType { T_DOUBLE, T_INT, T_UINT, T_FLOAT, T_SHORT, T_USHORT, T_UCHAR, T_UNKNOWN };
int field_size(FieldType t) {
    switch (t) {
        case T_DOUBLE: return 8;
        case T_INT: case T_UINT: case T_FLOAT: return 4;
        case T_SHORT: case T_USHORT: return 2;
        case T_UCHAR: return 1;
        default: return -1;
    }
}
FieldType field_type(const std::string& s) {
    if (s == "double") return T_DOUBLE;
    if (s == "int") return T_INT;
    if (s == "uint") return T_UINT;
    if (s == "float") return T_FLOAT;
    if (s == "short") return T_SHORT;
    if (s == "ushort") return T_USHORT;
    if (s == "uchar") return T_UCHAR;
    return T_UNKNOWN;
}

struct PlyField {
    bool present = false;
    FieldType type = T_UNKNOWN;
    size_t offset = 0;
};

// PlyParserUtils.readVertex for one field: false = `undefined`
bool read_field(const uint8_t* row, const PlyField& f, double* out) {
    if (!f.present) return false;
    const uint8_t* p = row + f.offset;
    switch (f.type) {
        case T_FLOAT: { float v; memcpy(&v, p, 4); *out = v; return true; }
        case T_SHORT: { int16_t v; memcpy(&v, p, 2); *out = v; return true; }
        case T_USHORT: { uint16_t v; memcpy(&v, p, 2); *out = v; return true; }
        case T_INT: { int32_t v; memcpy(&v, p, 4); *out = v; return true; }
        case T_UINT: { uint32_t v; memcpy(&v, p, 4); *out = v; return true; }
        case T_UCHAR: *out = (double)*p / 255.0; return true;                          // normalize = true
        default: return false;                                                         // doubles are never read (:281-301)
    }
}

std::string trim(const std::string& s) {
    size_t b = 0, e = s.size();
    while (b < e && isspace((unsigned char)s[b])) b++;
    while (e > b && isspace((unsigned char)s[e - 1])) e--;
    return s.substr(b, e - b);
}

// What the header of an INRIA-v1 PLY says: where the rows start, their stride and count, the output degree and where the fields
// the reference reads lie in a row.
struct PlyV1Header {
    size_t header_bytes = 0, bytes_per_vertex = 0;
    uint32_t vertex_count = 0, out_degree = 0;
    PlyField scale[3], rot[4], pos[3], dc[3], op, rgb[3], rest0, d1[9], d2[15];
};

// The header work of parse_ply, for the whole-file reader and the stream.  `bytes` of `data` are present; file_bytes is the file's
// size (what the rows are checked against) or STREAM_SIZE_UNKNOWN.  STREAM_NEED_MORE: no end_header yet, and more may come.
int ply_v1_header(const uint8_t* data, size_t bytes, size_t file_bytes, uint32_t want_degree, PlyV1Header& h) {
    const std::string token = "end_header";
    const std::string head((const char*)data, bytes < (1u << 20) ? bytes : (1u << 20));
    const size_t tok = head.find(token);
    if (tok == std::string::npos && bytes < (1u << 20) && bytes < file_bytes) return STREAM_NEED_MORE;
    GS_REQUIRE(tok != std::string::npos, "PLY: end_header not found");
    const size_t header_bytes = tok + token.size() + 1;                                // INRIAV1PlyParser.js:53
    // decodeSectionHeader: first `element` section only
    std::vector<std::pair<std::string, FieldType>> fields;
    uint32_t vertex_count = 0;
    bool in_section = false;
    size_t pos = 0;
    while (pos < tok + token.size()) {
        size_t nl = head.find('\n', pos);
        if (nl == std::string::npos) nl = head.size();
        const std::string line = trim(head.substr(pos, nl - pos));
        pos = nl + 1;
        if (line.rfind("element", 0) == 0) {
            if (in_section) break;
            in_section = true;
            size_t p1 = line.find_first_not_of(' ', 7);                                // components split on ' '
            size_t p2 = line.find(' ', p1);
            size_t p3 = p2 == std::string::npos ? p2 : line.find_first_not_of(' ', p2);
            if (p3 != std::string::npos) vertex_count = (uint32_t)strtoul(line.c_str() + p3, nullptr, 10);
        } else if (line.rfind("property", 0) == 0) {
            char w0[64], w1[64], w2[128];
            if (sscanf(line.c_str(), "%63[A-Za-z0-9_] %63[A-Za-z0-9_] %127[A-Za-z0-9_]", w0, w1, w2) == 3)     // /(\\w+)\\s+(\\w+)\\s+(\\w+)/
                fields.push_back({w2, field_type(w1)});
        }
        if (line == token) break;
    }
    size_t bytes_per_vertex = 0;
    uint32_t f_rest = 0;
    for (auto& f : fields) {
        GS_REQUIRE(field_size(f.second) > 0, "PLY: property type the reference does not size (bytesPerVertex would be NaN)");
        if (f.first.rfind("f_rest", 0) == 0) f_rest++;
    }
    // INRIAV1PlyParser.decodeHeaderLines: how many f_rest_* fields enter the name->id map
    const uint32_t sh_to_read = f_rest >= 45 ? 45u : (f_rest >= 24 ? 24u : (f_rest >= 9 ? 9u : 0u));
    auto mapped = [&](const std::string& name) {
        static const char* base[] = {"scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "x", "y", "z", "f_dc_0",
                                     "f_dc_1", "f_dc_2", "opacity", "red", "green", "blue", "f_rest_0"};
        for (const char* b : base)
            if (name == b) return true;
        if (name.rfind("f_rest_", 0) == 0) {
            const unsigned long k = strtoul(name.c_str() + 7, nullptr, 10);
            return k >= 1 && k + 1 <= sh_to_read && name == "f_rest_" + std::to_string(k);
        }
        return false;
    };
    auto find = [&](const std::string& name) {
        PlyField r;
        size_t off = 0;
        for (auto& f : fields) {
            if (f.first == name && mapped(name)) {                                     // later duplicates overwrite: keep the last
                r.present = true;
                r.type = f.second;
                r.offset = off;
            }
            off += (size_t)field_size(f.second);
        }
        return r;
    };
    for (auto& f : fields) bytes_per_vertex += (size_t)field_size(f.second);
    const double cpc_d = (double)f_rest / 3.0;                                         // coefficientsPerChannel (may be fractional)
    uint32_t degree = 0;
    if (cpc_d >= 3) degree = 1;
    if (cpc_d >= 8) degree = 2;
    const uint32_t out_degree = want_degree < degree ? want_degree : degree;
    GS_REQUIRE(file_bytes == STREAM_SIZE_UNKNOWN || header_bytes + bytes_per_vertex * (size_t)vertex_count <= file_bytes,
               "PLY: vertex data exceeds the file");
    PlyField(&F_scale)[3] = h.scale, (&F_rot)[4] = h.rot, (&F_pos)[3] = h.pos, (&F_dc)[3] = h.dc, &F_op = h.op, (&F_rgb)[3] = h.rgb,
            &F_rest0 = h.rest0, (&F_d1)[9] = h.d1, (&F_d2)[15] = h.d2;
    for (int k = 0; k < 3; k++) F_scale[k] = find("scale_" + std::to_string(k));
    for (int k = 0; k < 4; k++) F_rot[k] = find("rot_" + std::to_string(k));
    F_pos[0] = find("x"); F_pos[1] = find("y"); F_pos[2] = find("z");
    for (int k = 0; k < 3; k++) F_dc[k] = find("f_dc_" + std::to_string(k));
    F_op = find("opacity");
    F_rgb[0] = find("red"); F_rgb[1] = find("green"); F_rgb[2] = find("blue");
    F_rest0 = find("f_rest_0");
    // decodeSphericalHarmonicsFromSectionHeader: 'f_rest_' + (i + cpc*rgb [+ 3]); JS number -> string
    auto rest_name = [&](double k) {
        char t[64];
        if (k == floor(k)) snprintf(t, sizeof(t), "f_rest_%.0f", k);
        else snprintf(t, sizeof(t), "f_rest_%.17g", k);
        return std::string(t);
    };
    for (int rgb = 0; rgb < 3; rgb++) {
        if (degree >= 1) for (int i = 0; i < 3; i++) F_d1[3 * rgb + i] = find(rest_name(i + cpc_d * rgb));
        if (degree >= 2) for (int i = 0; i < 5; i++) F_d2[5 * rgb + i] = find(rest_name(i + cpc_d * rgb + 3));
    }
    h.header_bytes = header_bytes;
    h.bytes_per_vertex = bytes_per_vertex;
    h.vertex_count = vertex_count;
    h.out_degree = out_degree;
    return GS_OK;
}

int parse_ply(gs_asset* a, const uint8_t* data, size_t bytes, uint32_t want_degree) {
    PlyV1Header h;
    GS_TRY(ply_v1_header(data, bytes, bytes, want_degree, h));
    const size_t header_bytes = h.header_bytes, bytes_per_vertex = h.bytes_per_vertex;
    const uint32_t vertex_count = h.vertex_count, out_degree = h.out_degree;
    const PlyField(&F_scale)[3] = h.scale, (&F_rot)[4] = h.rot, (&F_pos)[3] = h.pos, (&F_dc)[3] = h.dc, &F_op = h.op, (&F_rgb)[3] = h.rgb,
                  &F_rest0 = h.rest0, (&F_d1)[9] = h.d1, (&F_d2)[15] = h.d2;
    const uint32_t ncomp = sh_components(out_degree), bps = 44u + 4u * ncomp;
    level0_header(a->buf, vertex_count, out_degree);
    uint8_t* B = a->buf.data() + KS_HEADER + KS_SECTION_HEADER;
    const uint8_t* rows = data + header_bytes;
    for (uint32_t i = 0; i < vertex_count; i++) {
        const uint8_t* row = rows + (size_t)i * bytes_per_vertex;
        uint8_t* o = B + (size_t)i * bps;
        Level0Tuple t;
        double v, s3[3], r4[4] = {NAN, NAN, NAN, NAN}, c3[3] = {NAN, NAN, NAN}, col[3], op = 0.0;   // createSplat() starts every field at 0
        // INRIAV1PlyParser.js:148-156
        if (read_field(row, F_scale[0], &v)) {
            for (int k = 0; k < 3; k++) { s3[k] = NAN; if (read_field(row, F_scale[k], &v)) s3[k] = exp(v); }
        } else {
            s3[0] = s3[1] = s3[2] = 0.01;
        }
        // :158-172
        if (read_field(row, F_dc[0], &v)) {
            const double SH_C0 = 0.28209479177387814;
            for (int k = 0; k < 3; k++) { col[k] = NAN; if (read_field(row, F_dc[k], &v)) col[k] = (0.5 + SH_C0 * v) * 255; }
        } else if (read_field(row, F_rgb[0], &v)) {
            for (int k = 0; k < 3; k++) { col[k] = NAN; if (read_field(row, F_rgb[k], &v)) col[k] = v * 255; }
        } else {
            col[0] = col[1] = col[2] = 0;
        }
        if (read_field(row, F_op, &v)) op = (1 / (1 + exp(-v))) * 255;                 // :174-176
        for (int k = 0; k < 3; k++) col[k] = clampd(floor(col[k]), 0, 255);            // :178-181
        op = clampd(floor(op), 0, 255);
        // :196-202 Quaternion.set(rot_0..3).normalize(), then the second normalize of writeSplatDataToSectionBuffer :1084-1086
        for (int k = 0; k < 4; k++) if (read_field(row, F_rot[k], &v)) r4[k] = v;
        row_normalize(r4);
        row_normalize(r4);
        for (int k = 0; k < 3; k++) if (read_field(row, F_pos[k], &v)) c3[k] = v;
        for (int k = 0; k < 3; k++) t.c[k] = (float)c3[k];
        for (int k = 0; k < 3; k++) t.s[k] = (float)(s3[k] == s3[k] ? s3[k] : 0.0);        // `|| 0`
        for (int k = 0; k < 4; k++) t.r[k] = (float)r4[k];
        for (int k = 0; k < 3; k++) t.rgba[k] = clamped_u8(col[k]);
        t.rgba[3] = clamped_u8(op);
        store_level0_row(o, t);
        if (out_degree >= 1) {                                                         // :183-194
            const bool have = read_field(row, F_rest0, &v);
            for (int s = 0; s < 9; s++) {
                double c = 0;
                if (have && read_field(row, F_d1[s], &v)) c = v;
                store_level0_sh(o, s, (float)c);
            }
            if (out_degree >= 2)
                for (int s = 0; s < 15; s++) {
                    double c = 0;
                    if (have && read_field(row, F_d2[s], &v)) c = v;
                    store_level0_sh(o, 9 + s, (float)c);
                }
        }
    }
    return parse_ksplat(a);
}

// What a host fill of a .splat / compressed PLY / .spz / INRIA-v2 PLY asset reads: every file row through the shared row arithmetic
// (asset_internal.hpp) into the level-0 row the reference stores for it.  Built once, on the first fill.
// the level-0 row (44 + 4 * ncomp bytes at o) of splat i of an asset that keeps file rows
void level0_row_of(const gs_asset* a, uint32_t i, uint32_t ncomp, uint8_t* o) {
    Level0Tuple t;
    if (a->rows == ASSET_ROWS_SPLAT) {
        uint32_t w[8];
        memcpy(w, a->file.data() + 32 * (size_t)i, 32);
        splat_row_tuple(w, t);
    } else if (a->rows == ASSET_ROWS_SPZ) {
        const SpzLayout& L = a->spz;
        const uint8_t* f = a->file.data();
        auto three = [&](int plane) {
            const uint8_t* p = f + L.off[plane] + 3 * (size_t)i;
            return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        };
        SpzRowBytes b;
        const uint8_t* pp = f + L.off[SPZ_POSITIONS] + (size_t)L.pos_stride * i;
        for (int k = 0; k < 3; k++)
            b.pos[k] = L.pos_stride == 9u ? ((uint32_t)pp[3 * k] | ((uint32_t)pp[3 * k + 1] << 8) | ((uint32_t)pp[3 * k + 2] << 16))
                                          : ((uint32_t)pp[2 * k] | ((uint32_t)pp[2 * k + 1] << 8));
        b.alpha = f[L.off[SPZ_ALPHAS] + i];
        b.colour = three(SPZ_COLOURS); b.scale = three(SPZ_SCALES); b.rotation = three(SPZ_ROTATIONS);
        spz_row_tuple(L, b, t);
        const uint8_t* sh = f + L.off[SPZ_SH] + 3 * (size_t)L.file_dim * i;
        for (uint32_t s = 0; s < ncomp; s++) store_level0_sh(o, s, spz_sh_value(sh[spz_sh_index(s)]));
    } else if (a->rows == ASSET_ROWS_INRIA_V1) {
        const uint8_t* row = a->file.data() + a->iv1_vertex_base + (size_t)a->iv1.stride * i;
        inria_v1_row_tuple(row, a->iv1, t);
        const bool has_sh = inria_v1_row_has_sh(row, a->iv1);
        for (uint32_t s = 0; s < ncomp; s++) store_level0_sh(o, s, inria_v1_row_sh(row, a->iv1, has_sh, s));
    } else if (a->rows == ASSET_ROWS_INRIA_V2) {
        const uint8_t* row = a->file.data() + a->iv2_vertex_base + (size_t)a->iv2.stride * i;
        inria_v2_row_tuple(row, a->iv2, a->iv2_codebook.data(), t);
        for (uint32_t s = 0; s < ncomp; s++) store_level0_sh(o, s, inria_v2_row_sh(row, a->iv2, a->iv2_codebook.data(), s));
    } else {
        uint32_t w[4];
        memcpy(w, a->file.data() + a->pc_vertex_base + 16 * (size_t)i, 16);
        pc_row_tuple(w, a->file.data() + a->pc_chunk_base + (size_t)a->pc.chunk_stride * (i / 256u), a->pc, t);
        const uint8_t* sh = a->file.data() + a->pc_sh_base + (size_t)a->pc.sh_stride * i;
        for (uint32_t s = 0; s < ncomp; s++) store_level0_sh(o, s, pc_row_sh(sh, a->pc.read_coeff, s));
    }
    store_level0_row(o, t);
}

int build_level0_image(gs_asset* a) {
    if (a->rows == ASSET_ROWS_KSPLAT || !a->buf.empty()) return GS_OK;
    const uint32_t n = a->splat_count, degree = a->sh_degree, ncomp = sh_components(degree), bps = 44u + 4u * ncomp;
    level0_header(a->buf, n, degree);
    uint8_t* B = a->buf.data() + KS_HEADER + KS_SECTION_HEADER;
    for (uint32_t i = 0; i < n; i++) level0_row_of(a, i, ncomp, B + (size_t)i * bps);
    const int st = parse_ksplat(a);
    if (st != GS_OK) a->buf.clear();
    return st;
}

int check_splat_bytes(size_t bytes) {
    GS_REQUIRE(bytes % 32 == 0, ".splat: the byte count is not a multiple of the 32-byte row");
    GS_REQUIRE(bytes / 32 <= 0xFFFFFFFFull, ".splat: more than 2^32 - 1 rows");
    return GS_OK;
}
void parse_splat_rows(gs_asset* a, size_t bytes) {           // `bytes` passed check_splat_bytes
    a->rows = ASSET_ROWS_SPLAT;
    a->splat_count = (uint32_t)(bytes / 32);
    a->level = 0;
    a->sh_degree = 0;
}
int parse_splat(gs_asset* a, const uint8_t* data, size_t bytes) {
    GS_TRY(check_splat_bytes(bytes));
    a->file.assign(data, data + bytes);
    parse_splat_rows(a, bytes);
    return GS_OK;
}

// .spz: the gzip member is inflated and checked at open (spz_container.hpp: the stream is exactly header + planes, so every
// plane byte of every splat exists); the asset keeps the inflated stream, never the gzip.
int parse_spz(gs_asset* a, const uint8_t* data, size_t bytes, uint32_t want_degree) {
    SpzHeader h;
    const char* refusal = spz_open(data, bytes, a->file, h);
    GS_REQUIRE(refusal == nullptr, refusal);
    uint32_t degree = want_degree < h.sh_degree ? want_degree : h.sh_degree;           // Math.min(file, out) :370
    if (degree > 2) degree = 2;                                                        // the level-0 row holds two bands
    a->rows = ASSET_ROWS_SPZ;
    a->spz = h.layout;
    a->splat_count = h.count;
    a->level = 0;
    a->sh_degree = degree;
    return GS_OK;
}

// PlyParserUtils.determineHeaderFormatFromHeaderText: every trimmed header line is looked at, the LAST match decides
enum PlyFlavour { PLY_INRIA_V1, PLY_COMPRESSED, PLY_INRIA_V2 };
// settled (a stream asks): no byte that may still follow changes the answer - the end_header line is in, newline included, or the
// 1 MiB that is looked at is.
PlyFlavour ply_flavour(const uint8_t* data, size_t bytes, bool* settled = nullptr) {
    const std::string head((const char*)data, bytes < (1u << 20) ? bytes : (1u << 20));
    PlyFlavour f = PLY_INRIA_V1;
    size_t pos = 0;
    if (settled) *settled = bytes >= (1u << 20);
    while (pos < head.size()) {
        size_t nl = head.find('\n', pos);
        const bool ended = nl != std::string::npos;
        if (nl == std::string::npos) nl = head.size();
        const std::string line = trim(head.substr(pos, nl - pos));
        pos = nl + 1;
        if (line.rfind("element chunk", 0) == 0 || line.find("packed_") != std::string::npos) f = PLY_COMPRESSED;
        else if (line.rfind("element codebook_centers", 0) == 0) f = PLY_INRIA_V2;
        else if (line == "end_header") {
            if (settled && ended) *settled = true;
            break;
        }
    }
    return f;
}

// decodeHeader + decodeHeaderText.  The reference is memory-safe JavaScript and reads whatever the header describes; here
// the layout the row decode relies on is proven at open: chunk, vertex[, sh] in that order (readPly reads them in that order
// whatever the header says), sixteen-byte vertex rows of the four packed uints, float extremes, one uchar per SH property,
// enough chunks, and every element inside the file.
// What the header says (everything of the asset but the bytes).  `bytes` of `data` are present; file_bytes is the file's size (what
// the elements are checked against) or STREAM_SIZE_UNKNOWN.  STREAM_NEED_MORE: the header's end is not among the bytes, and more
// may come.
struct PcHeader {
    PcLayout layout;
    size_t base[3];                // chunk, vertex, sh
    bool has_sh;
    uint32_t chunk_count, splat_count, degree;
};
int compressed_ply_header(const uint8_t* data, size_t bytes, size_t file_bytes, uint32_t want_degree, PcHeader& out) {
    static const char end_token[] = "\nend_header\n";
    GS_REQUIRE(bytes >= 4 && memcmp(data, "ply\n", 4) == 0, "compressed PLY: the file does not start with 'ply'");
    const uint8_t* e = std::search(data, data + bytes, (const uint8_t*)end_token, (const uint8_t*)end_token + 12);
    if (e == data + bytes && bytes < file_bytes) return STREAM_NEED_MORE;
    GS_REQUIRE(e != data + bytes, "compressed PLY: end of header not found");
    const std::string text((const char*)data, (size_t)(e - data));
    const size_t header_bytes = (size_t)(e - data) + 12;
    struct Prop { std::string type, name; uint32_t size; };
    struct Element { std::string name; uint64_t count; std::vector<Prop> props; uint64_t stride = 0; };
    std::vector<Element> elements;
    size_t pos = text.find('\n');                                                       // line 0 ("ply") is not looked at
    pos = pos == std::string::npos ? text.size() : pos + 1;
    while (pos < text.size()) {
        size_t nl = text.find('\n', pos);
        if (nl == std::string::npos) nl = text.size();
        const std::string line = text.substr(pos, nl - pos);
        pos = nl + 1;
        if (line.rfind("comment ", 0) == 0) continue;
        std::vector<std::string> words;                                                // String.split(' ')
        for (size_t b = 0;;) {
            const size_t sp = line.find(' ', b);
            words.push_back(line.substr(b, sp == std::string::npos ? sp : sp - b));
            if (sp == std::string::npos) break;
            b = sp + 1;
        }
        while (words.size() < 3) words.push_back("");
        if (words[0] == "format") {
            GS_REQUIRE(words[1] == "binary_little_endian", "compressed PLY: the format is not binary_little_endian");
        } else if (words[0] == "element") {
            Element el;
            el.name = words[1];
            const std::string& c = words[2];                                           // parseInt(words[2], 10)
            size_t d = 0;
            uint64_t v = 0;
            while (d < c.size() && c[d] >= '0' && c[d] <= '9' && v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(c[d++] - '0');
            GS_REQUIRE(d > 0 && v <= 0xFFFFFFFFull, "compressed PLY: an element count is not a number below 2^32");
            el.count = v;
            elements.push_back(el);
        } else if (words[0] == "property") {
            static const struct { const char* name; uint32_t size; } types[] = {{"char", 1}, {"uchar", 1}, {"short", 2}, {"ushort", 2},
                                                                               {"int", 4}, {"uint", 4}, {"float", 4}, {"double", 8}};
            uint32_t size = 0;
            for (auto& t : types) if (words[1] == t.name) size = t.size;
            GS_REQUIRE(size != 0, "compressed PLY: unrecognized property data type");
            GS_REQUIRE(!elements.empty(), "compressed PLY: a property precedes every element");
            elements.back().props.push_back({words[1], words[2], size});
            elements.back().stride += size;
        } else {
            GS_REQUIRE(false, "compressed PLY: unrecognized header value (only format / element / property lines are read)");
        }
    }
    GS_REQUIRE(elements.size() >= 2 && elements[0].name == "chunk" && elements[1].name == "vertex",
               "compressed PLY: the elements must begin with chunk, vertex");
    const Element &chunk = elements[0], &vertex = elements[1];
    const Element* sh = elements.size() >= 3 && elements[2].name == "sh" ? &elements[2] : nullptr;
    for (size_t k = 2; k < elements.size(); k++)
        GS_REQUIRE(elements[k].name != "chunk" && elements[k].name != "vertex" && (elements[k].name != "sh" || k == 2),
                   "compressed PLY: a chunk / vertex / sh element is repeated or out of order");
    size_t off = header_bytes;
    size_t base[3] = {0, 0, 0};
    for (size_t k = 0; k < elements.size(); k++) {                                     // every element lies inside the file
        if (k < 3) base[k] = off;
        const uint64_t need = elements[k].stride * elements[k].count;                  // < 2^32 * (8 * lines of a 2^40 header): no overflow
        GS_REQUIRE(elements[k].stride < (1ull << 24), "compressed PLY: an element row of 16 MiB or more");
        GS_REQUIRE(file_bytes == STREAM_SIZE_UNKNOWN || (off <= file_bytes && need <= file_bytes - off),
                   "compressed PLY: element data exceeds the file");
        off += (size_t)need;
    }
    const uint64_t n = vertex.count;
    GS_REQUIRE(chunk.count >= (n + 255) / 256, "compressed PLY: fewer chunks than ceil(vertex count / 256)");
    PcLayout L = {};
    {
        static const char* packed[4] = {"packed_position", "packed_rotation", "packed_scale", "packed_color"};
        GS_REQUIRE(vertex.props.size() == 4 && vertex.stride == 16, "compressed PLY: a vertex row is not the four packed uints");
        for (int w = 0; w < 4; w++) {
            int at = -1;
            for (int k = 3; k >= 0; k--) if (vertex.props[k].name == packed[w]) at = k;
            GS_REQUIRE(at >= 0 && vertex.props[at].type == "uint", "compressed PLY: a packed_* property is missing or not uint");
            L.word[w] = (uint32_t)at;
        }
    }
    {
        static const char* names[18] = {"min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                                        "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"};
        bool aligned = chunk.stride % 4 == 0;
        for (int w = 0; w < 18; w++) {
            L.ext[w] = -1;
            uint32_t o = 0;
            for (const Prop& p : chunk.props) {                                        // Array.find: the first of that name
                if (p.name == names[w]) {
                    GS_REQUIRE(p.type == "float", "compressed PLY: a chunk extreme is not float");
                    L.ext[w] = (int32_t)o;
                    aligned = aligned && o % 4 == 0;
                    break;
                }
                o += p.size;
            }
            GS_REQUIRE(w >= 12 || L.ext[w] >= 0, "compressed PLY: a position / scale extreme is missing from the chunk element");
        }
        L.chunk_stride = (uint32_t)chunk.stride;
        L.chunk_aligned = aligned ? 1u : 0u;
    }
    uint32_t file_degree = 0;
    if (sh) {
        GS_REQUIRE(sh->count == n, "compressed PLY: the sh element's count differs from the vertex count");
        const size_t P = sh->props.size();
        for (size_t k = 0; k < P; k++)
            GS_REQUIRE(sh->props[k].type == "uchar" && sh->props[k].name == "f_rest_" + std::to_string(k),
                       "compressed PLY: the sh element is not f_rest_0 .. f_rest_N-1 as uchar");
        file_degree = P >= 45 ? 3u : (P >= 24 ? 2u : (P >= 9 ? 1u : 0u));
        L.sh_stride = (uint32_t)P;
        L.read_coeff = file_degree == 3 ? 15u : (file_degree == 2 ? 8u : (file_degree == 1 ? 3u : 0u));
    }
    uint32_t degree = want_degree < file_degree ? want_degree : file_degree;            // Math.min(out, file)
    if (degree > 2) degree = 2;                                                        // the level-0 row holds two bands
    out.layout = L;
    for (int k = 0; k < 3; k++) out.base[k] = base[k];
    out.has_sh = sh != nullptr;
    out.chunk_count = (uint32_t)chunk.count;
    out.splat_count = (uint32_t)n;
    out.degree = degree;
    return GS_OK;
}

void adopt_compressed_ply(gs_asset* a, const PcHeader& h) {
    a->rows = ASSET_ROWS_COMPRESSED_PLY;
    a->pc = h.layout;
    a->pc_chunk_base = h.base[0];
    a->pc_vertex_base = h.base[1];
    a->pc_sh_base = h.has_sh ? h.base[2] : 0;
    a->pc_chunk_count = h.chunk_count;
    a->splat_count = h.splat_count;
    a->level = 0;
    a->sh_degree = h.degree;
}

int parse_compressed_ply(gs_asset* a, const uint8_t* data, size_t bytes, uint32_t want_degree) {
    PcHeader h;
    GS_TRY(compressed_ply_header(data, bytes, bytes, want_degree, h));
    a->file.assign(data, data + bytes);
    adopt_compressed_ply(a, h);
    return GS_OK;
}

// ---- INRIA-v2 codebook PLY ---------------------------------------------------------------------------------------------------
// One entry of the decoded codebook (asset_internal.hpp says what a row does with it): fromHalfFloat, decodeCodeBook's rule for the
// page (INRIAV2PlyParser.js:143-158), then what parseToUncompressedSplat (:206-237) and the level-0 store (SplatBuffer.js:1100-1121,
// 1169-1170) do to a value whatever the row: floor, clamp 0..255, `|| 0`, fp32.  Math.exp is row_exp, as for the compressed PLY.
float inria_v2_decode_entry(uint32_t page, uint16_t half) {
    const double v = from_half(half), SH_C0 = 0.28209479177387814;
    if (page == IV2_PAGE_DC || page == IV2_PAGE_OPACITY) {
        const double c = page == IV2_PAGE_DC ? js_round((0.5 + SH_C0 * v) * 255) : js_round((1 / (1 + row_exp(-v))) * 255);
        return (float)clamped_u8(clampd(floor(c), 0, 255));
    }
    if (page == IV2_PAGE_SCALING) {
        const double e = row_exp(v);
        return (float)(e == e ? e : 0.0);
    }
    if (page >= IV2_PAGE_REST) return v == v && v != 0 ? (float)v : 0.0f;              // `|| 0`: NaN and -0 become +0
    return row_f32(v);                                                                 // rotation_re / rotation_im
}

// decodeHeaderFromBuffer + decodeCodeBook.  The sections are decoded as PlyParserUtils.decodeSectionHeader decodes them (trimmed lines,
// /(\w+)\s+(\w+)\s+(\w+)/ on property lines, later duplicates of a name overwrite earlier ones, anything but element / property lines is
// dropped).  The reference is memory-safe JavaScript and turns whatever the header describes into undefined / NaN; here everything the
// row decode relies on is proven at open, and what the reference would make every splat NaN of is refused.
int parse_inria_v2(gs_asset* a, const uint8_t* data, size_t bytes, uint32_t want_degree) {
    const std::string token = "end_header";
    const std::string head((const char*)data, bytes < (1u << 20) ? bytes : (1u << 20));
    const size_t tok = head.find(token);
    GS_REQUIRE(tok != std::string::npos, "INRIA-v2 PLY: end_header not found");
    const size_t header_bytes = tok + token.size() + 1;                                // INRIAV2PlyParser.js:104
    struct Prop { std::string name; FieldType type; uint32_t offset; };
    struct Section { std::string name; uint64_t count = 0, stride = 0; std::vector<Prop> props; size_t base = 0; };
    std::vector<Section> sections;
    for (size_t pos = 0; pos < tok + token.size();) {
        size_t nl = head.find('\n', pos);
        if (nl == std::string::npos) nl = head.size();
        const std::string line = trim(head.substr(pos, nl - pos));
        pos = nl + 1;
        if (line == token) break;
        if (line.rfind("format", 0) == 0) {
            GS_REQUIRE(line.rfind("format binary_little_endian", 0) == 0, "INRIA-v2 PLY: the format is not binary_little_endian");
        } else if (line.rfind("element", 0) == 0) {
            char name[128], count[32];
            if (sscanf(line.c_str(), "element %127s %31s", name, count) != 2) name[0] = count[0] = 0;
            uint64_t v = 0;
            size_t d = 0;
            while (count[d] >= '0' && count[d] <= '9' && v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(count[d++] - '0');
            GS_REQUIRE(d > 0 && v <= 0xFFFFFFFFull, "INRIA-v2 PLY: an element count is not a number below 2^32");
            sections.emplace_back();
            sections.back().name = name;
            sections.back().count = v;
        } else if (line.rfind("property", 0) == 0) {
            char w0[64], w1[64], w2[128];
            if (sscanf(line.c_str(), "%63[A-Za-z0-9_] %63[A-Za-z0-9_] %127[A-Za-z0-9_]", w0, w1, w2) != 3) continue;
            const FieldType type = field_type(w1);
            GS_REQUIRE(field_size(type) > 0, "INRIA-v2 PLY: property type the reference does not size (bytesPerVertex would be NaN)");
            GS_REQUIRE(!sections.empty(), "INRIA-v2 PLY: a property precedes every element");
            Section& sec = sections.back();
            GS_REQUIRE(sec.stride + (uint64_t)field_size(type) < (1u << 16), "INRIA-v2 PLY: an element row of 64 KiB or more");
            sec.props.push_back({w2, type, (uint32_t)sec.stride});
            sec.stride += (uint64_t)field_size(type);
        }
    }
    const Section *book = nullptr, *vertex = nullptr;
    size_t off = header_bytes;
    for (Section& sec : sections) {                                                    // findVertexData: the elements' rows follow in header order
        GS_REQUIRE(off <= bytes && sec.stride * sec.count <= bytes - off, "INRIA-v2 PLY: element data exceeds the file");
        sec.base = off;
        off += (size_t)(sec.stride * sec.count);
        const Section*& slot = sec.name == "codebook_centers" ? book : vertex;
        GS_REQUIRE(slot == nullptr, "INRIA-v2 PLY: more than one codebook_centers element, or more than one element besides it");
        slot = &sec;
    }
    GS_REQUIRE(book != nullptr, "INRIA-v2 PLY: no codebook_centers element");
    GS_REQUIRE(vertex != nullptr, "INRIA-v2 PLY: no element besides codebook_centers");
    GS_REQUIRE(book->count >= 256, "INRIA-v2 PLY: fewer than 256 codebook rows (an index byte reaches any of 256)");

    // ---- the vertex element: which byte of a row is which attribute's index
    auto starts = [](const std::string& s, const char* prefix) { return s.rfind(prefix, 0) == 0; };
    uint32_t f_rest = 0;
    for (const Prop& p : vertex->props) {
        if (p.name == "x" || p.name == "y" || p.name == "z")
            GS_REQUIRE(p.type == T_SHORT || p.type == T_USHORT, "INRIA-v2 PLY: x / y / z are not short / ushort (half bits)");
        if (starts(p.name, "f_dc_") || starts(p.name, "f_rest") || starts(p.name, "scale_") || starts(p.name, "rot_") || p.name == "opacity")
            GS_REQUIRE(p.type == T_UCHAR, "INRIA-v2 PLY: an index field (f_dc_* / f_rest_* / opacity / scale_* / rot_*) is not uchar");
        if (starts(p.name, "f_rest")) f_rest++;
    }
    GS_REQUIRE(f_rest == 0 || f_rest == 9 || f_rest == 24 || f_rest == 45, "INRIA-v2 PLY: the f_rest_* fields are not 0, 9, 24 or 45");
    const uint32_t cpc = f_rest / 3, file_degree = cpc >= 8 ? 2u : (cpc >= 3 ? 1u : 0u);
    auto find = [](const Section& sec, const std::string& name) {
        uint16_t at = IV2_ABSENT;
        for (const Prop& p : sec.props) if (p.name == name) at = (uint16_t)p.offset;    // later duplicates overwrite: keep the last
        return at;
    };
    InriaV2Layout L = {};
    L.stride = (uint32_t)vertex->stride;
    L.pos[0] = find(*vertex, "x"); L.pos[1] = find(*vertex, "y"); L.pos[2] = find(*vertex, "z");
    for (int k = 0; k < 4; k++) L.rot[k] = find(*vertex, "rot_" + std::to_string(k));
    for (int k = 0; k < 3; k++) {
        GS_REQUIRE(L.pos[k] != IV2_ABSENT, "INRIA-v2 PLY: x / y / z missing (the reference makes every centre NaN)");
        L.scale[k] = find(*vertex, "scale_" + std::to_string(k));
        L.dc[k] = find(*vertex, "f_dc_" + std::to_string(k));
    }
    for (int k = 0; k < 4; k++) GS_REQUIRE(L.rot[k] != IV2_ABSENT, "INRIA-v2 PLY: rot_0 .. rot_3 missing (the reference makes every rotation NaN)");
    L.opacity = find(*vertex, "opacity");
    for (uint32_t s = 0; s < 24; s++) {                                                // decodeSphericalHarmonicsFromSectionHeader, in level-0 slot order
        const uint32_t k = s < 9 ? s % 3 + cpc * (s / 3) : 3 + (s - 9) % 5 + cpc * ((s - 9) / 5);
        L.sh[s] = s < sh_components(file_degree) ? find(*vertex, "f_rest_" + std::to_string(k)) : (uint16_t)IV2_ABSENT;
    }

    // ---- the codebook: the pages the file's fields reach must exist as half bits; pages nothing reaches stay 0
    static const char* const rest_names[15] = {"features_rest_0", "features_rest_1", "features_rest_2", "features_rest_3", "features_rest_4",
                                               "features_rest_5", "features_rest_6", "features_rest_7", "features_rest_8", "features_rest_9",
                                               "features_rest_10", "features_rest_11", "features_rest_12", "features_rest_13", "features_rest_14"};
    const char* page_name[IV2_PAGES] = {"features_dc", "opacity", "scaling", "rotation_re", "rotation_im"};
    bool needed[IV2_PAGES] = {L.dc[0] != IV2_ABSENT, L.opacity != IV2_ABSENT, L.scale[0] != IV2_ABSENT, true, true};
    for (uint32_t k = 0; k < 15; k++) {
        page_name[IV2_PAGE_REST + k] = rest_names[k];
        needed[IV2_PAGE_REST + k] = k < (file_degree == 0 ? 0u : (file_degree == 1 ? 3u : 8u));
    }
    a->iv2_codebook.assign((size_t)IV2_PAGES * 256, 0.0f);
    for (uint32_t page = 0; page < IV2_PAGES; page++) {
        const Prop* prop = nullptr;
        for (const Prop& p : book->props) if (p.name == page_name[page]) prop = &p;
        GS_REQUIRE(prop || !needed[page], "INRIA-v2 PLY: a codebook page that the file's fields need is missing");
        if (!prop) continue;
        GS_REQUIRE(prop->type == T_SHORT || prop->type == T_USHORT, "INRIA-v2 PLY: a codebook property is not short / ushort (half bits)");
        for (uint32_t i = 0; i < 256; i++) {
            uint16_t h;
            memcpy(&h, data + book->base + (size_t)book->stride * i + prop->offset, 2);
            a->iv2_codebook[256 * page + i] = inria_v2_decode_entry(page, h);
        }
    }
    uint32_t degree = want_degree < file_degree ? want_degree : file_degree;           // Math.min(out, file) :203; the level-0 row holds two bands
    if (data != a->file.data()) a->file.assign(data, data + bytes);                     // (a stream's bytes are there already)
    a->rows = ASSET_ROWS_INRIA_V2;
    a->iv2 = L;
    a->iv2_vertex_base = vertex->base;
    a->splat_count = (uint32_t)vertex->count;
    a->level = 0;
    a->sh_degree = degree;
    return GS_OK;
}

// ---- streamed assets: gs_asset_open_stream / gs_asset_append (the byte counting is asset_stream.cpp) ---------------------------------
// the one copy of the stream's bytes: the vector an opened asset of the format keeps its file in (.spz: the gzip member, apart)
std::vector<uint8_t>& stream_bytes(gs_asset* a) {
    const uint32_t format = a->stream->format;
    return format == GS_ASSET_KSPLAT ? a->buf : (format == GS_ASSET_SPZ ? a->stream->raw : a->file);
}

// parse_ply's fields as the row arithmetic of both sides reads them (asset_internal.hpp)
InriaV1Layout inria_v1_layout(const PlyV1Header& h) {
    InriaV1Layout L = {};
    L.stride = (uint32_t)h.bytes_per_vertex;
    bool aligned = L.stride % 4u == 0;
    auto field = [&](const PlyField& f) {
        InriaV1Field o = {0, 0, 0};
        uint8_t type;
        switch (f.type) {
            case T_FLOAT: type = IV1_FLOAT; break;
            case T_INT: type = IV1_INT; break;
            case T_UINT: type = IV1_UINT; break;
            case T_SHORT: type = IV1_SHORT; break;
            case T_USHORT: type = IV1_USHORT; break;
            case T_UCHAR: type = IV1_UCHAR; break;
            default: return o;                                                         // doubles are never read: as absent
        }
        if (!f.present) return o;
        o = {(uint16_t)f.offset, type, 1};
        if (type <= IV1_UINT && f.offset % 4 != 0) aligned = false;
        return o;
    };
    for (int k = 0; k < 3; k++) { L.pos[k] = field(h.pos[k]); L.scale[k] = field(h.scale[k]); L.dc[k] = field(h.dc[k]); L.rgb[k] = field(h.rgb[k]); }
    for (int k = 0; k < 4; k++) L.rot[k] = field(h.rot[k]);
    L.opacity = field(h.op);
    L.rest0 = field(h.rest0);
    for (int k = 0; k < 9; k++) L.sh[k] = field(h.d1[k]);
    for (int k = 0; k < 15; k++) L.sh[9 + k] = field(h.d2[k]);
    L.aligned = aligned ? 1u : 0u;
    return L;
}

// The bytes of an append are in: what the format's reader makes of the prefix (final: of the file).  < 0: the append is refused.
int stream_step(gs_asset* a, bool final) {
    AssetStream& s = *a->stream;
    std::vector<uint8_t>& store = stream_bytes(a);
    const uint8_t* data = store.data();
    const size_t n = store.size(), file_bytes = final ? n : STREAM_SIZE_UNKNOWN;
    size_t implied = 0;                                       // the file's size as the header implies it (0: not known)
    const bool had_header = s.header_ready;
    if (s.format == GS_ASSET_SPLAT) {
        GS_REQUIRE(!final || n == s.expected_bytes, ".splat: the stream ended before expected_bytes had arrived");
    } else if (s.format == GS_ASSET_KSPLAT) {
        std::vector<StreamRun> runs;
        const int st = parse_ksplat(a, false, &runs, &implied);
        if (st < 0) return st;
        if (st == STREAM_NEED_MORE) {
            if (final) return parse_ksplat(a);                // too short for its headers: the whole-file reader's refusal
        } else {
            if (a->sh_degree > s.max_sh_degree) a->sh_degree = s.max_sh_degree;
            s.header_ready = true;
            s.splat_limit = a->splat_count;
            s.runs.swap(runs);
            GS_REQUIRE(!final || implied <= n, KS_DATA_EXCEEDS);
        }
    } else if (s.format == GS_ASSET_SPZ) {                    // a gzip member with a trailing CRC: nothing before the end
        if (final) {
            GS_TRY(parse_spz(a, data, n, s.max_sh_degree));
            std::vector<uint8_t>().swap(s.raw);
        }
    } else if (!s.header_ready || final) {                    // PLY: the header, once it is in; again at the end, against the file's size
        bool settled = false;
        const PlyFlavour flavour = ply_flavour(data, n, &settled);
        if (!settled && !final) {
        } else if (flavour == PLY_INRIA_V2) {                 // the codebook may follow the rows: nothing before the end
            if (final) GS_TRY(parse_inria_v2(a, data, n, s.max_sh_degree));
        } else if (flavour == PLY_COMPRESSED) {
            PcHeader h;
            const int st = compressed_ply_header(data, n, file_bytes, s.max_sh_degree, h);
            if (st < 0) return st;
            if (st != STREAM_NEED_MORE) {
                adopt_compressed_ply(a, h);
                // a splat reads its vertex row, its chunk row and - above degree 0 - its SH row: the chunk element is the gate,
                // and the SH element, which lies behind every vertex row, arrives last
                const bool sh = h.degree > 0;
                s.runs.assign(1, {(uint64_t)h.base[1], (uint64_t)(sh ? h.base[2] : h.base[1]), sh ? h.layout.sh_stride : 16u, 0u, h.splat_count});
                implied = (h.has_sh ? h.base[2] + (size_t)h.layout.sh_stride * h.splat_count : h.base[1] + 16 * (size_t)h.splat_count);
                s.header_ready = true;
            }
        } else {
            PlyV1Header h;
            const int st = ply_v1_header(data, n, file_bytes, s.max_sh_degree, h);
            if (st < 0) return st;
            if (st != STREAM_NEED_MORE) {
                GS_REQUIRE(h.bytes_per_vertex < (1u << 16), "PLY: a vertex row of 64 KiB or more");
                a->rows = ASSET_ROWS_INRIA_V1;
                a->iv1 = inria_v1_layout(h);
                a->iv1_vertex_base = h.header_bytes;
                a->splat_count = h.vertex_count;
                a->level = 0;
                a->sh_degree = h.out_degree;
                s.runs.assign(1, {(uint64_t)h.header_bytes, (uint64_t)h.header_bytes, (uint32_t)h.bytes_per_vertex, 0u, h.vertex_count});
                implied = h.header_bytes + h.bytes_per_vertex * (size_t)h.vertex_count;
                s.header_ready = true;
            }
        }
        s.splat_limit = a->splat_count;
    }
    if (s.header_ready && !had_header && implied > store.capacity() && !final) {
        try {
            store.reserve(implied);                           // the size the header implies, now that it is known
        } catch (const std::exception&) {                     // (a header may imply anything: the vector then grows as the bytes come)
        }
    }
    if (final) s.finish(n, a->splat_count);
    else s.advance(n);
    return GS_OK;
}

// gs_asset_fill's loop: every splat of the image through the shared per-splat body (asset_internal.hpp)
template <bool XF>
void fill_image(const gs_asset* a, uint32_t min_alpha, float* centers, float* cov_f32, uint16_t* cov_f16, uint8_t* rgba, uint16_t* sh_f16,
                uint8_t* sh_u8, float* scales, float* rotations) {
    const KsplatSource image = a->image();
    const AssetTransform xf = a->xf;                       // a local: the byte stores of the loop cannot be taken to change it
    const double sh_min = a->sh_min, sh_max = a->sh_max;
    for (uint32_t i = 0, n = a->splat_count; i < n; i++)
        asset_fill_splat<XF, true>(image.row(i), xf, image.sh_degree, image.ncomp, sh_min, sh_max, min_alpha, i, centers, cov_f32, cov_f16,
                                   rgba, sh_f16, sh_u8, scales, rotations);
}

}  // namespace

extern "C" {

int gs_asset_open(const void* data, uint64_t bytes, uint32_t format, uint32_t max_sh_degree, gs_asset** out) {
    GS_REQUIRE(data && out, "data / out == NULL");
    *out = nullptr;
    gs_asset* a = new (std::nothrow) gs_asset();
    if (!a) return GS_ERR_NOMEM;
    int st;
    try {
        if (format == GS_ASSET_PLY) {
            const PlyFlavour flavour = ply_flavour((const uint8_t*)data, (size_t)bytes);
            if (flavour == PLY_INRIA_V2) {
                st = parse_inria_v2(a, (const uint8_t*)data, (size_t)bytes, max_sh_degree);
            } else if (flavour == PLY_COMPRESSED) {
                st = parse_compressed_ply(a, (const uint8_t*)data, (size_t)bytes, max_sh_degree);
            } else {
                st = parse_ply(a, (const uint8_t*)data, (size_t)bytes, max_sh_degree);
            }
        } else if (format == GS_ASSET_SPLAT) {
            st = parse_splat(a, (const uint8_t*)data, (size_t)bytes);
        } else if (format == GS_ASSET_SPZ) {
            st = parse_spz(a, (const uint8_t*)data, (size_t)bytes, max_sh_degree);
        } else if (format == GS_ASSET_KSPLAT) {
            a->buf.assign((const uint8_t*)data, (const uint8_t*)data + bytes);
            st = parse_ksplat(a);
            if (st == GS_OK && a->sh_degree > max_sh_degree) a->sh_degree = max_sh_degree;
        } else {
            gs_set_error("invalid argument: unknown asset format");
            st = GS_ERR_INVALID;
        }
    } catch (const std::bad_alloc&) {
        gs_set_error("out of host memory while reading the asset");
        st = GS_ERR_NOMEM;
    }
    if (st != GS_OK) {
        delete a;
        return st;
    }
    *out = a;
    return GS_OK;
}

void gs_asset_close(gs_asset* a) { delete a; }

int gs_asset_open_stream(uint32_t format, uint32_t max_sh_degree, uint64_t expected_bytes, gs_asset** out) {
    GS_REQUIRE(out != nullptr, "out == NULL");
    *out = nullptr;
    GS_REQUIRE(format == GS_ASSET_PLY || format == GS_ASSET_KSPLAT || format == GS_ASSET_SPLAT || format == GS_ASSET_SPZ, "unknown asset format");
    if (format == GS_ASSET_SPLAT) {
        GS_REQUIRE(expected_bytes != 0, ".splat: a stream needs expected_bytes (the splat count comes from it)");
        GS_TRY(check_splat_bytes((size_t)expected_bytes));
    }
    gs_asset* a = new (std::nothrow) gs_asset();
    if (!a) return GS_ERR_NOMEM;
    try {
        a->stream.reset(new AssetStream());
        AssetStream& s = *a->stream;
        s.format = format;
        s.max_sh_degree = max_sh_degree;
        s.expected_bytes = expected_bytes;
        stream_bytes(a).reserve((size_t)expected_bytes);
        if (format == GS_ASSET_SPLAT) {                       // no header: everything is known now
            s.bounded = true;
            parse_splat_rows(a, (size_t)expected_bytes);
            s.header_ready = true;
            s.splat_limit = a->splat_count;
            s.runs.push_back({0, 0, 32u, 0u, a->splat_count});
        }
    } catch (const std::exception&) {                         // bad_alloc, length_error
        delete a;
        gs_set_error("out of host memory while reserving the stream's bytes");
        return GS_ERR_NOMEM;
    }
    *out = a;
    return GS_OK;
}

int gs_asset_append(gs_asset* a, const void* data, uint64_t bytes, int final) {
    GS_REQUIRE(a != nullptr, "asset == NULL");
    GS_REQUIRE(a->stream != nullptr, "the asset is no stream (gs_asset_open_stream opens one)");
    GS_REQUIRE(data || bytes == 0, "data == NULL");
    AssetStream& s = *a->stream;
    const char* refusal = s.admit(bytes);
    if (refusal) {
        s.refuse();
        GS_REQUIRE(false, refusal);
    }
    std::vector<uint8_t>& store = stream_bytes(a);
    const size_t before = store.size();
    int st;
    try {
        store.insert(store.end(), (const uint8_t*)data, (const uint8_t*)data + bytes);
        st = stream_step(a, final != 0);
    } catch (const std::bad_alloc&) {
        gs_set_error("out of host memory while reading the stream");
        st = GS_ERR_NOMEM;
    }
    if (st < 0) {
        store.resize(before);                                 // nothing of a refused append is consumed
        s.refuse();
        return st;
    }
    return GS_OK;
}

int gs_asset_get_stream_info(gs_asset* a, gs_asset_stream_info* info) {
    GS_REQUIRE(a && info, "asset / info == NULL");
    GS_REQUIRE(a->stream != nullptr, "the asset is no stream (gs_asset_open_stream opens one)");
    const AssetStream& s = *a->stream;
    info->bytes_received = s.bytes_received;
    info->header_ready = s.header_ready;
    info->splats_ready = s.splats_ready;
    info->complete = s.complete;
    info->failed = s.failed;
    return GS_OK;
}

// Debug entry for the tests (pure host; not in the public header): splat `splat` of the READY prefix as the host reads it out of
// the bytes that have arrived - the level-0 row (44 + 4 * ncomp bytes) an asset of file rows decodes it to, or, for a .ksplat image,
// the float centre (through the bucket tables) followed by the rest of the file row.  out holds GS_DEBUG_ASSET_ROW_BYTES (140: a
// level-0 row of degree 2, the longest of either kind); *bytes says how many were written.
int gs_debug_asset_row(gs_asset* a, uint32_t splat, void* out, uint32_t* bytes) {
    GS_REQUIRE(a && out && bytes, "asset / out / bytes == NULL");
    GS_REQUIRE(splat < a->ready(), "the splat is not ready");
    uint8_t* o = (uint8_t*)out;
    if (a->rows != ASSET_ROWS_KSPLAT) {
        const uint32_t ncomp = sh_components(a->sh_degree);
        level0_row_of(a, splat, ncomp, o);
        *bytes = 44u + 4u * ncomp;
        return GS_OK;
    }
    const KsplatSource image = a->image();
    const KsplatSource::Row row = image.row(splat);
    double d[3];
    row.centre(d);
    for (int k = 0; k < 3; k++) { const float c = (float)d[k]; memcpy(o + 4 * k, &c, 4); }
    const uint32_t rest = row.sec.bytes_per_splat - asset_center_bytes(a->level);
    memcpy(o + 12, row.srow(), rest);
    *bytes = 12u + rest;
    return GS_OK;
}

int gs_asset_get_info(gs_asset* a, gs_asset_info* info) {
    GS_REQUIRE(a && info, "asset / info == NULL");
    GS_REQUIRE(!a->stream || a->stream->header_ready, "the stream's header has not arrived (gs_asset_stream_info.header_ready)");
    info->splat_count = a->splat_count;
    info->sh_degree = a->sh_degree;
    info->compression_level = a->level;
    info->sh_level = a->level < 1 ? 1u : a->level;          // getTargetSphericalHarmonicsCompressionLevel
    for (int k = 0; k < 3; k++) info->scene_center[k] = a->scene_center[k];
    info->sh_min = (float)a->sh_min;
    info->sh_max = (float)a->sh_max;
    return GS_OK;
}

int gs_asset_fill(gs_asset* a, uint32_t min_alpha, float* centers, float* cov_f32, uint16_t* cov_f16, uint8_t* rgba,
                  uint16_t* sh_f16, uint8_t* sh_u8, float* scales, float* rotations) {
    GS_REQUIRE(a != nullptr, "asset == NULL");
    GS_REQUIRE(!a->incomplete(), "the stream is not complete: gs_asset_fill reads the whole file (uploads take the ready prefix)");
    GS_REQUIRE(!(sh_f16 && sh_u8), "pass sh_f16 (compression level <= 1) or sh_u8 (level 2), not both");
    GS_REQUIRE(!sh_u8 || a->level == 2, "sh_u8 output needs a compression level 2 file (SplatMesh.js:1064-1066)");
    GS_REQUIRE(!sh_f16 || a->level <= 1, "a level 2 file keeps its SH as uint8: ask for sh_u8");
    GS_REQUIRE(!a->has_transform || !(scales || rotations),
               "scales / rotations of a transformed asset are not provided (gs_asset_set_transform(a, NULL) removes the transform)");
    try {
        GS_TRY(build_level0_image(a));                       // .splat / compressed PLY / .spz: the first fill lays the level-0 rows out
    } catch (const std::bad_alloc&) {
        gs_set_error("out of host memory while decoding the asset");
        return GS_ERR_NOMEM;
    }
    if (a->has_transform) fill_image<true>(a, min_alpha, centers, cov_f32, cov_f16, rgba, sh_f16, sh_u8, scales, rotations);
    else fill_image<false>(a, min_alpha, centers, cov_f32, cov_f16, rgba, sh_f16, sh_u8, scales, rotations);
    return GS_OK;
}

// The per-call preamble of the transformed fills, done once (SplatBuffer.js:628-637 and the band-2 rows of
// rotateSphericalHarmonics5 :775-815, which the reference recomputes per splat from the same inputs).
int gs_asset_set_transform(gs_asset* a, const double* transform16) {
    GS_REQUIRE(a != nullptr, "asset == NULL");
    if (!transform16) {
        a->has_transform = false;
        return GS_OK;
    }
    const double* te = transform16;
    for (int k = 0; k < 16; k++) GS_REQUIRE(isfinite(te[k]), "scene transform: an element is not finite");
    GS_REQUIRE(te[3] == 0 && te[7] == 0 && te[11] == 0 && te[15] == 1, "scene transform: the bottom row is not (0, 0, 0, 1)");
    // Matrix4.decompose (three r160)
    double sx = sqrt(te[0] * te[0] + te[1] * te[1] + te[2] * te[2]);
    const double sy = sqrt(te[4] * te[4] + te[5] * te[5] + te[6] * te[6]);
    const double sz = sqrt(te[8] * te[8] + te[9] * te[9] + te[10] * te[10]);
    GS_REQUIRE(sx != 0 && sy != 0 && sz != 0, "scene transform: a basis column has length 0 (Matrix4.decompose divides by it)");
    {   // Matrix4.determinant
        const double n11 = te[0], n12 = te[4], n13 = te[8], n14 = te[12], n21 = te[1], n22 = te[5], n23 = te[9], n24 = te[13];
        const double n31 = te[2], n32 = te[6], n33 = te[10], n34 = te[14], n41 = te[3], n42 = te[7], n43 = te[11], n44 = te[15];
        const double det =
            n41 * (+n14 * n23 * n32 - n13 * n24 * n32 - n14 * n22 * n33 + n12 * n24 * n33 + n13 * n22 * n34 - n12 * n23 * n34) +
            n42 * (+n11 * n23 * n34 - n11 * n24 * n33 + n14 * n21 * n33 - n13 * n21 * n34 + n13 * n24 * n31 - n14 * n23 * n31) +
            n43 * (+n11 * n24 * n32 - n11 * n22 * n34 - n14 * n21 * n32 + n12 * n21 * n34 + n14 * n22 * n31 - n12 * n24 * n31) +
            n44 * (-n13 * n22 * n31 - n11 * n23 * n32 + n11 * n22 * n33 + n13 * n21 * n32 - n12 * n21 * n33 + n12 * n23 * n31);
        if (det < 0) sx = -sx;
    }
    const double invSX = 1 / sx, invSY = 1 / sy, invSZ = 1 / sz;
    const double m11 = te[0] * invSX, m21 = te[1] * invSX, m31 = te[2] * invSX;
    const double m12 = te[4] * invSY, m22 = te[5] * invSY, m32 = te[6] * invSY;
    const double m13 = te[8] * invSZ, m23 = te[9] * invSZ, m33 = te[10] * invSZ;
    // Quaternion.setFromRotationMatrix
    double qx, qy, qz, qw;
    const double trace = m11 + m22 + m33;
    if (trace > 0) {
        const double s = 0.5 / sqrt(trace + 1.0);
        qw = 0.25 / s; qx = (m32 - m23) * s; qy = (m13 - m31) * s; qz = (m21 - m12) * s;
    } else if (m11 > m22 && m11 > m33) {
        const double s = 2.0 * sqrt(1.0 + m11 - m22 - m33);
        qw = (m32 - m23) / s; qx = 0.25 * s; qy = (m12 + m21) / s; qz = (m13 + m31) / s;
    } else if (m22 > m33) {
        const double s = 2.0 * sqrt(1.0 + m22 - m11 - m33);
        qw = (m13 - m31) / s; qx = (m12 + m21) / s; qy = 0.25 * s; qz = (m23 + m32) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + m33 - m11 - m22);
        qw = (m21 - m12) / s; qx = (m13 + m31) / s; qy = (m23 + m32) / s; qz = 0.25 * s;
    }
    double q[4] = {qx, qy, qz, qw};
    row_normalize(q);                                                                  // tempRotation.normalize()
    // makeRotationFromQuaternion = compose(zero, q, one), then Matrix3.setFromMatrix4: E = Matrix3.elements (column-major)
    double E[9];
    {
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double x2 = x + x, y2 = y + y, z2 = z + z;
        const double xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2;
        const double wx = w * x2, wy = w * y2, wz = w * z2;
        E[0] = (1 - (yy + zz)) * 1; E[1] = (xy + wz) * 1; E[2] = (xz - wy) * 1;
        E[3] = (xy - wz) * 1; E[4] = (1 - (xx + zz)) * 1; E[5] = (yz + wx) * 1;
        E[6] = (xz + wy) * 1; E[7] = (yz - wx) * 1; E[8] = (1 - (xx + yy)) * 1;
    }
    AssetTransform t;
    for (int k = 0; k < 16; k++) t.m[k] = te[k];
    double(&sh11)[3] = t.sh1[0], (&sh12)[3] = t.sh1[1], (&sh13)[3] = t.sh1[2];
    sh11[0] = E[4]; sh11[1] = -E[7]; sh11[2] = E[1];                                    // SplatBuffer.js:634-636
    sh12[0] = -E[5]; sh12[1] = E[8]; sh12[2] = -E[2];
    sh13[0] = E[3]; sh13[1] = -E[6]; sh13[2] = E[0];
    const double kSqrt0104 = sqrt(1.0 / 4.0), kSqrt0304 = sqrt(3.0 / 4.0), kSqrt0103 = sqrt(1.0 / 3.0), kSqrt0403 = sqrt(4.0 / 3.0),
                 kSqrt0112 = sqrt(1.0 / 12.0);
    double(&sh21)[5] = t.sh2[0], (&sh22)[5] = t.sh2[1], (&sh23)[5] = t.sh2[2], (&sh24)[5] = t.sh2[3], (&sh25)[5] = t.sh2[4];
    sh21[0] = kSqrt0104 * ((sh13[2] * sh11[0] + sh13[0] * sh11[2]) + (sh11[2] * sh13[0] + sh11[0] * sh13[2]));   // :781-815
    sh21[1] = (sh13[1] * sh11[0] + sh11[1] * sh13[0]);
    sh21[2] = kSqrt0304 * (sh13[1] * sh11[1] + sh11[1] * sh13[1]);
    sh21[3] = (sh13[1] * sh11[2] + sh11[1] * sh13[2]);
    sh21[4] = kSqrt0104 * ((sh13[2] * sh11[2] - sh13[0] * sh11[0]) + (sh11[2] * sh13[2] - sh11[0] * sh13[0]));
    sh22[0] = kSqrt0104 * ((sh12[2] * sh11[0] + sh12[0] * sh11[2]) + (sh11[2] * sh12[0] + sh11[0] * sh12[2]));
    sh22[1] = sh12[1] * sh11[0] + sh11[1] * sh12[0];
    sh22[2] = kSqrt0304 * (sh12[1] * sh11[1] + sh11[1] * sh12[1]);
    sh22[3] = sh12[1] * sh11[2] + sh11[1] * sh12[2];
    sh22[4] = kSqrt0104 * ((sh12[2] * sh11[2] - sh12[0] * sh11[0]) + (sh11[2] * sh12[2] - sh11[0] * sh12[0]));
    sh23[0] = kSqrt0103 * (sh12[2] * sh12[0] + sh12[0] * sh12[2]) +
              -kSqrt0112 * ((sh13[2] * sh13[0] + sh13[0] * sh13[2]) + (sh11[2] * sh11[0] + sh11[0] * sh11[2]));
    sh23[1] = kSqrt0403 * sh12[1] * sh12[0] + -kSqrt0103 * (sh13[1] * sh13[0] + sh11[1] * sh11[0]);
    sh23[2] = sh12[1] * sh12[1] + -kSqrt0104 * (sh13[1] * sh13[1] + sh11[1] * sh11[1]);
    sh23[3] = kSqrt0403 * sh12[1] * sh12[2] + -kSqrt0103 * (sh13[1] * sh13[2] + sh11[1] * sh11[2]);
    sh23[4] = kSqrt0103 * (sh12[2] * sh12[2] - sh12[0] * sh12[0]) +
              -kSqrt0112 * ((sh13[2] * sh13[2] - sh13[0] * sh13[0]) + (sh11[2] * sh11[2] - sh11[0] * sh11[0]));
    sh24[0] = kSqrt0104 * ((sh12[2] * sh13[0] + sh12[0] * sh13[2]) + (sh13[2] * sh12[0] + sh13[0] * sh12[2]));
    sh24[1] = sh12[1] * sh13[0] + sh13[1] * sh12[0];
    sh24[2] = kSqrt0304 * (sh12[1] * sh13[1] + sh13[1] * sh12[1]);
    sh24[3] = sh12[1] * sh13[2] + sh13[1] * sh12[2];
    sh24[4] = kSqrt0104 * ((sh12[2] * sh13[2] - sh12[0] * sh13[0]) + (sh13[2] * sh12[2] - sh13[0] * sh12[0]));
    sh25[0] = kSqrt0104 * ((sh13[2] * sh13[0] + sh13[0] * sh13[2]) - (sh11[2] * sh11[0] + sh11[0] * sh11[2]));
    sh25[1] = (sh13[1] * sh13[0] - sh11[1] * sh11[0]);
    sh25[2] = kSqrt0304 * (sh13[1] * sh13[1] - sh11[1] * sh11[1]);
    sh25[3] = (sh13[1] * sh13[2] - sh11[1] * sh11[2]);
    sh25[4] = kSqrt0104 * ((sh13[2] * sh13[2] - sh13[0] * sh13[0]) - (sh11[2] * sh11[2] - sh11[0] * sh11[0]));
    a->xf = t;
    a->has_transform = true;
    return GS_OK;
}

}  // extern "C"
