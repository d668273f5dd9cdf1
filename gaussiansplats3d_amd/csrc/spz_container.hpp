// spz_container.hpp — the .spz container, host side: a gzip member (RFC 1952) around a deflate stream (RFC 1951) around a
// 16-byte header and six byte planes.  Includes nothing of HIP: a plain C++17 compiler builds it (tests/tools/spz_sanitize.cpp
// does, under AddressSanitizer and UBSan), and the library needs no zlib.  Restates, never copies:
//   container         src/loaders/spz/SpzLoader.js:255-342 (deserializePackedGaussians): header fields, plane order, every refusal
//   position scale    SpzLoader.js:184 `1.0 / (1 << fractionalBits)` with JavaScript's shift: the count is taken mod 32 and the
//                     result is an int32, so 31 gives -2^31 (a NEGATIVE scale) and 40 behaves as 8.  Reproduced.
// The reference inflates through the browser's DecompressionStream and then dies on a null `packed` for every container it
// refuses; here each refusal is a message (spz_open returns it, NULL = success).
// Every read and write is bounded: the bit reader never passes the end of the input, a match never reaches before the start
// of the output, and the output is capped - at the 16 header bytes until those are known, then at exactly the length the
// header implies.  A stream that would produce one byte more, or that ends short, is refused.
// A DECISION, not a restatement: bytes behind the member's trailer (a second member included) are refused.  Browsers'
// DecompressionStream errors on trailing data; a Node stand-in built on zlib.gunzipSync cannot show that either way.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

// Where a splat's bytes lie in the inflated stream.  Plain data: it is also the device decode's kernel argument.
enum { SPZ_POSITIONS = 0, SPZ_ALPHAS = 1, SPZ_COLOURS = 2, SPZ_SCALES = 3, SPZ_ROTATIONS = 4, SPZ_SH = 5, SPZ_PLANES = 6 };
struct SpzLayout {
    uint32_t off[SPZ_PLANES];  // byte offset of each plane in the inflated stream, in file order (the enum above)
    uint32_t pos_stride;       // 9 (version 2: three 24-bit fixed-point values) or 6 (version 1: three halves)
    uint32_t file_dim;         // SH coefficients per channel in the file: 0 / 3 / 8 / 15
    double pos_scale;          // version 2: 1.0 / (1 << fractionalBits), JavaScript's shift
};

struct SpzHeader {
    uint32_t version, count, sh_degree, fractional_bits, flags;
    uint64_t stream_bytes;     // 16 + every plane
    SpzLayout layout;
};

constexpr uint32_t SPZ_MAGIC = 1347635022u, SPZ_HEADER_BYTES = 16u, SPZ_MAX_POINTS = 10000000u;

inline uint32_t spz_dim_for_degree(uint32_t degree) { return degree == 0 ? 0u : (degree == 1 ? 3u : (degree == 2 ? 8u : 15u)); }
inline uint32_t spz_plane_stride(const SpzLayout& L, int plane) {
    return plane == SPZ_POSITIONS ? L.pos_stride : (plane == SPZ_ALPHAS ? 1u : (plane == SPZ_SH ? 3u * L.file_dim : 3u));
}

// The 16 header bytes -> what the reference's checks let through, and the exact length of the stream that must follow
inline const char* spz_parse_header(const uint8_t h[16], SpzHeader& out) {
    auto u32 = [&](int o) { return (uint32_t)h[o] | ((uint32_t)h[o + 1] << 8) | ((uint32_t)h[o + 2] << 16) | ((uint32_t)h[o + 3] << 24); };
    if (u32(0) != SPZ_MAGIC) return ".spz: wrong magic (the inflated stream does not start with the SPZ header)";
    out.version = u32(4);
    if (out.version < 1 || out.version > 2) return ".spz: version not supported (1 and 2 are)";
    out.count = u32(8);
    if (out.count > SPZ_MAX_POINTS) return ".spz: too many points (numPoints above 10 000 000)";
    out.sh_degree = h[12];
    if (out.sh_degree > 3) return ".spz: unsupported SH degree (shDegree above 3)";
    out.fractional_bits = h[13];
    out.flags = h[14];                                   // bit 0 = antialiased: parsed and dropped, as the reference does
    SpzLayout& L = out.layout;
    L.pos_stride = out.version == 1 ? 6u : 9u;
    L.file_dim = spz_dim_for_degree(out.sh_degree);
    L.pos_scale = 1.0 / (double)(int32_t)(1u << (out.fractional_bits & 31u));
    uint64_t at = SPZ_HEADER_BYTES;                      // at most 16 + 10^7 * 64: below 2^32
    for (int p = 0; p < SPZ_PLANES; p++) {
        L.off[p] = (uint32_t)at;
        at += (uint64_t)spz_plane_stride(L, p) * out.count;
    }
    out.stream_bytes = at;
    return nullptr;
}

namespace spz_detail {

struct Crc32 {
    uint32_t t[8][256];
    Crc32() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 8; s++) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 255u];
    }
    uint32_t operator()(const uint8_t* p, size_t n) const {
        uint32_t c = 0xFFFFFFFFu;
        for (; n >= 8; n -= 8, p += 8) {
            const uint32_t a = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
            c = t[7][a & 255u] ^ t[6][(a >> 8) & 255u] ^ t[5][(a >> 16) & 255u] ^ t[4][a >> 24] ^ t[3][p[4]] ^ t[2][p[5]] ^ t[1][p[6]] ^
                t[0][p[7]];
        }
        for (; n; n--, p++) c = (c >> 8) ^ t[0][(c ^ *p) & 255u];
        return c ^ 0xFFFFFFFFu;
    }
};

// LSB-first bit reader over [in, in + n): `fill` takes what is there, `take` refuses more bits than are left
struct Bits {
    const uint8_t* in;
    size_t n, pos = 0;
    uint64_t acc = 0;
    uint32_t cnt = 0;
    void fill() {
        while (cnt <= 56 && pos < n) { acc |= (uint64_t)in[pos++] << cnt; cnt += 8; }
    }
    bool take(uint32_t bits, uint32_t& v) {              // bits <= 16
        if (cnt < bits) fill();
        if (cnt < bits) return false;
        v = (uint32_t)(acc & ((1ull << bits) - 1ull));
        acc >>= bits;
        cnt -= bits;
        return true;
    }
    void align() {                                       // to the next byte boundary, whole bytes handed back
        const uint32_t drop = cnt & 7u;
        acc >>= drop;
        cnt -= drop;
        pos -= cnt / 8u;
        acc = 0;
        cnt = 0;
    }
};

// A canonical Huffman code (RFC 1951 3.2.2): codes of up to FAST bits through a table indexed by the next bits of the
// stream (stored bit-reversed, as the stream carries codes most significant bit first), longer ones length by length.
struct Huffman {
    enum { FAST = 10, MAXBITS = 15 };
    uint16_t fast[1 << FAST];      // (symbol << 4) | length, 0 = not a short code
    uint16_t count[MAXBITS + 1], symbol[288];
    uint16_t first_code[MAXBITS + 2], first_index[MAXBITS + 2];

    // false: over-subscribed, or incomplete.  Let through, as inflaters in use do: a single code of length 1 (RFC 1951 allows it
    // for distances) and no code at all (a block of literals only); a bit pattern outside such a code then fails in decode.
    bool build(const uint8_t* lengths, uint32_t n) {
        memset(fast, 0, sizeof(fast));
        memset(count, 0, sizeof(count));
        for (uint32_t s = 0; s < n; s++) count[lengths[s]]++;
        count[0] = 0;
        int left = 1;
        for (int l = 1; l <= MAXBITS; l++) {
            left = (left << 1) - (int)count[l];
            if (left < 0) return false;
        }
        uint32_t total = 0;
        for (int l = 1; l <= MAXBITS; l++) total += count[l];
        if (left > 0 && total != 0 && !(total == 1 && count[1] == 1)) return false;
        uint16_t offs[MAXBITS + 2];
        uint32_t code = 0, index = 0;
        for (int l = 1; l <= MAXBITS; l++) {
            first_code[l] = (uint16_t)code;
            first_index[l] = offs[l] = (uint16_t)index;
            code = (code + count[l]) << 1;
            index += count[l];
        }
        for (uint32_t s = 0; s < n; s++)
            if (lengths[s]) symbol[offs[lengths[s]]++] = (uint16_t)s;
        for (int l = 1; l <= FAST; l++)
            for (uint32_t k = 0; k < count[l]; k++) {
                const uint32_t c = first_code[l] + k;
                uint32_t r = 0;
                for (int b = 0; b < l; b++) r |= ((c >> b) & 1u) << (l - 1 - b);
                for (uint32_t hi = r; hi < (1u << FAST); hi += 1u << l) fast[hi] = (uint16_t)((symbol[first_index[l] + k] << 4) | l);
            }
        return true;
    }
    // -1: no code matches, or the stream ends inside the code
    int decode(Bits& b) const {
        if (b.cnt < MAXBITS) b.fill();
        const uint16_t e = fast[b.acc & ((1u << FAST) - 1u)];
        if (e) {
            const uint32_t l = e & 15u;
            if (l > b.cnt) return -1;
            b.acc >>= l;
            b.cnt -= l;
            return e >> 4;
        }
        uint32_t code = 0;
        for (int l = 1; l <= MAXBITS; l++) {
            if ((uint32_t)l > b.cnt) return -1;
            code = (code << 1) | (uint32_t)((b.acc >> (l - 1)) & 1u);
            if (l > FAST && code >= first_code[l] && code - first_code[l] < count[l]) {
                b.acc >>= l;
                b.cnt -= l;
                return symbol[first_index[l] + (code - first_code[l])];
            }
        }
        return -1;
    }
};

// The output: capped at the 16 header bytes until the header is known, then sized once to what the header implies
struct Sink {
    std::vector<uint8_t> out;
    size_t size = 0, limit = SPZ_HEADER_BYTES;
    bool sized = false;
    SpzHeader header = {};
    const char* error = nullptr;

    bool know_header() {                                 // size == 16: the cap becomes the header's exact length
        error = spz_parse_header(out.data(), header);
        if (error) return false;
        sized = true;
        limit = (size_t)header.stream_bytes;
        out.resize(limit);
        return true;
    }
    bool room(size_t n) {                                // may n more bytes be written?
        if (n <= limit - size) return true;
        if (!sized && size == SPZ_HEADER_BYTES && know_header() && n <= limit - size) return true;
        if (!error) error = sized ? ".spz: the deflate stream produces more bytes than the header implies"
                                  : ".spz: the deflate stream runs past the 16 header bytes before they are complete";
        return false;
    }
    // bytes are written in pieces that never straddle the 16-byte cap: a piece is cut there so the header is parsed first
    bool write(const uint8_t* p, size_t n) {
        while (n) {
            size_t piece = n;
            if (!sized && size < SPZ_HEADER_BYTES && piece > SPZ_HEADER_BYTES - size) piece = SPZ_HEADER_BYTES - size;
            if (!room(piece)) return false;
            memcpy(out.data() + size, p, piece);
            size += piece;
            p += piece;
            n -= piece;
        }
        return true;
    }
    bool put(uint8_t byte) {                             // a literal: the common case first
        if (sized && size < limit) { out[size++] = byte; return true; }
        return write(&byte, 1);
    }
    bool copy(size_t distance, size_t n) {               // an LZ77 match: may overlap its own output
        if (distance == 0 || distance > size) {
            error = ".spz: a deflate match reaches before the start of the output";
            return false;
        }
        while (n) {
            size_t piece = n;
            if (!sized && size < SPZ_HEADER_BYTES && piece > SPZ_HEADER_BYTES - size) piece = SPZ_HEADER_BYTES - size;
            if (!room(piece)) return false;
            uint8_t* d = out.data() + size;              // (room may have resized: take the pointer afterwards)
            const uint8_t* s = d - distance;
            for (size_t k = 0; k < piece; k++) d[k] = s[k];
            size += piece;
            n -= piece;
        }
        return true;
    }
};

inline const char* inflate(Bits& b, Sink& sink) {
    static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                           8193, 12289, 16385, 24577};
    static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    static const char* SHORT = ".spz: the deflate stream ends short";
    Huffman lit, dist;
    for (;;) {
        uint32_t last, type;
        if (!b.take(1, last) || !b.take(2, type)) return SHORT;
        if (type == 0) {                                                               // stored
            b.align();
            if (b.n - b.pos < 4) return SHORT;
            const uint32_t len = (uint32_t)b.in[b.pos] | ((uint32_t)b.in[b.pos + 1] << 8);
            const uint32_t nlen = (uint32_t)b.in[b.pos + 2] | ((uint32_t)b.in[b.pos + 3] << 8);
            if ((len ^ nlen) != 0xFFFFu) return ".spz: a stored block's length and its complement disagree";
            b.pos += 4;
            if (b.n - b.pos < len) return SHORT;
            if (!sink.write(b.in + b.pos, len)) return sink.error;
            b.pos += len;
        } else if (type == 1 || type == 2) {
            uint8_t lengths[320];
            uint32_t nlit = 288, ndist = 30;
            if (type == 1) {                                                           // fixed codes (RFC 1951 3.2.6): 288 and 32
                ndist = 32;                                                            // symbols take part, 286.. and 30.. never occur
                for (int s = 0; s < 288; s++) lengths[s] = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
                for (int s = 0; s < 32; s++) lengths[288 + s] = 5;
            } else {                                                                   // dynamic codes (3.2.7)
                uint32_t hlit, hdist, hclen;
                if (!b.take(5, hlit) || !b.take(5, hdist) || !b.take(4, hclen)) return SHORT;
                nlit = hlit + 257;
                ndist = hdist + 1;
                if (nlit > 286 || ndist > 30) return ".spz: a dynamic block declares too many codes";
                uint8_t cl[19] = {0};
                for (uint32_t k = 0; k < hclen + 4; k++) {
                    uint32_t v;
                    if (!b.take(3, v)) return SHORT;
                    cl[ORDER[k]] = (uint8_t)v;
                }
                Huffman code;
                if (!code.build(cl, 19)) return ".spz: a dynamic block's code-length code is not a prefix code";
                uint32_t at = 0;
                while (at < nlit + ndist) {
                    const int s = code.decode(b);
                    if (s < 0) return ".spz: the deflate stream ends short or holds an unassigned code";
                    if (s < 16) { lengths[at++] = (uint8_t)s; continue; }
                    uint32_t rep, prev = 0;
                    if (s == 16) {
                        if (at == 0) return ".spz: a dynamic block repeats a code length before the first";
                        prev = lengths[at - 1];
                        if (!b.take(2, rep)) return SHORT;
                        rep += 3;
                    } else if (s == 17) {
                        if (!b.take(3, rep)) return SHORT;
                        rep += 3;
                    } else {
                        if (!b.take(7, rep)) return SHORT;
                        rep += 11;
                    }
                    if (at + rep > nlit + ndist) return ".spz: a dynamic block's code lengths overrun their count";
                    while (rep--) lengths[at++] = (uint8_t)prev;
                }
                if (lengths[256] == 0) return ".spz: a dynamic block has no end-of-block code";
                memmove(lengths + 288, lengths + nlit, ndist);                          // (nlit <= 286: moves upwards, regions may overlap)
            }
            if (!lit.build(lengths, nlit)) return ".spz: a block's literal/length code is not a prefix code";
            if (!dist.build(lengths + 288, ndist)) return ".spz: a block's distance code is not a prefix code";
            for (;;) {
                const int s = lit.decode(b);
                if (s < 0) return ".spz: the deflate stream ends short or holds an unassigned code";
                if (s < 256) {
                    if (!sink.put((uint8_t)s)) return sink.error;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return ".spz: a length symbol above 285";
                uint32_t extra;
                if (!b.take(LEN_EXTRA[s - 257], extra)) return SHORT;
                const uint32_t len = LEN_BASE[s - 257] + extra;
                const int d = dist.decode(b);
                if (d < 0) return ".spz: the deflate stream ends short or holds an unassigned code";
                if (d > 29) return ".spz: a distance symbol above 29";
                if (!b.take(DIST_EXTRA[d], extra)) return SHORT;
                if (!sink.copy((size_t)DIST_BASE[d] + extra, len)) return sink.error;
            }
        } else {
            return ".spz: a deflate block of the reserved type 3";
        }
        if (last) return nullptr;
    }
}

}  // namespace spz_detail

// gzip member -> the inflated SPZ stream (header + planes, exactly header.stream_bytes long) and its parsed header.
// Returns NULL, or the reason the file is refused.
inline const char* spz_open(const uint8_t* data, size_t n, std::vector<uint8_t>& stream, SpzHeader& header) {
    using namespace spz_detail;
    static const Crc32 crc;
    if (n < 10) return ".spz: shorter than a gzip header";
    if (data[0] != 0x1F || data[1] != 0x8B) return ".spz: not a gzip stream (the file does not start with 1f 8b)";
    if (data[2] != 8) return ".spz: the gzip compression method is not deflate";
    const uint32_t flg = data[3];
    if (flg & 0xE0u) return ".spz: reserved gzip flag bits are set";
    size_t pos = 10;                                                                   // MTIME, XFL and OS are not looked at
    if (flg & 4u) {                                                                    // FEXTRA
        if (n - pos < 2) return ".spz: the gzip header ends short";
        const size_t xlen = (size_t)data[pos] | ((size_t)data[pos + 1] << 8);
        pos += 2;
        if (n - pos < xlen) return ".spz: the gzip header ends short";
        pos += xlen;
    }
    for (uint32_t bit : {8u, 16u})                                                     // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (pos < n && data[pos] != 0) pos++;
            if (pos >= n) return ".spz: the gzip header ends short";
            pos++;
        }
    if (flg & 2u) {                                                                    // FHCRC: the low half of the header's CRC-32
        if (n - pos < 2) return ".spz: the gzip header ends short";
        const uint32_t want = (uint32_t)data[pos] | ((uint32_t)data[pos + 1] << 8);
        if ((crc(data, pos) & 0xFFFFu) != want) return ".spz: the gzip header's CRC-16 is wrong";
        pos += 2;
    }
    Bits bits{data + pos, n - pos};
    Sink sink;
    sink.out.resize(SPZ_HEADER_BYTES);
    if (const char* e = inflate(bits, sink)) return e;
    if (sink.size < SPZ_HEADER_BYTES) return ".spz: the inflated stream is shorter than the 16-byte SPZ header";
    if (!sink.sized && !sink.know_header()) return sink.error;
    if (sink.size != sink.limit) return ".spz: incorrect size (the inflated stream ends before the planes the header implies)";
    bits.align();
    const uint8_t* t = bits.in + bits.pos;
    const size_t left = bits.n - bits.pos;
    if (left < 8) return ".spz: the gzip trailer is cut short";
    auto u32 = [&](int o) { return (uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24); };
    if (u32(0) != crc(sink.out.data(), sink.size)) return ".spz: wrong CRC-32 in the gzip trailer";
    if (u32(4) != (uint32_t)(sink.size & 0xFFFFFFFFu)) return ".spz: wrong ISIZE in the gzip trailer";
    if (left != 8) return ".spz: trailing bytes behind the gzip member's trailer";
    stream.swap(sink.out);
    header = sink.header;
    return nullptr;
}
