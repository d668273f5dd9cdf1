// bin_word.hpp — the binner's look-up word: what k_project leaves per splat POSITION of a live storage block (ProjSet::prect) and
// k_bin_count gathers once per sorted index: {visible, record slot in the block, 16-px tile rect}.  The ONLY place that knows
// either layout; host and device (draw_plan.cpp's debug entry packs and unpacks on the host, tests/test_bin_word.py).
//
// Two words, one per draw (draw_plan.hpp, narrow_bin_word):
//   wide    8 bytes  {x0:12 | y0:12 | slot:8,  x1:12 | y1:12 | visible:1}                  any frame up to 4096 x 4096 tiles
//   narrow  4 bytes  x0:8 | y0:8 | (x1 - x0):4 | (y1 - y0):4 | slot:8                      frames of <= 256 x 256 tiles
//     spans 0 .. 14 are direct.  Span code 15 in x marks what the word cannot say:
//       x span 15, y span 15   not visible (slot and origin are zero: the word is BIN_WORD_INVISIBLE)
//       x span 15, y span 0    ESCAPE: visible, the word carries the slot only and the rect is ProjSet::rects[block base + slot] of the
//                              SAME record set - the 16-px rect k_project writes per record for the blend.  A span above 14 or a
//                              coordinate above 255 escapes (C3: 0.36 % of the visible splats, a 4K frame of tiny splats 4e-7).
//     A direct word never has x span 15, so no visible splat encodes to the invisible code.
// The gather's cost is the table's footprint in the live blocks (profiles/r12_gather_live_blocks.txt), hence the narrow word.
#pragma once
#include <stdint.h>

#if defined(__HIP__)       // (the attributes spelled out: draw_plan.cpp includes no HIP header)
#define GS_BIN_WORD_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GS_BIN_WORD_FN inline
#endif

// a rect as the kernels carry it: lo = x0 | y0 << 16, hi = x1 | y1 << 16 (16-px tiles, inclusive)
struct BinRect { uint32_t lo, hi; };
struct BinWordWide { uint32_t x, y; };
struct BinWordOut {
    bool visible, escape;          // escape: `rect` is not set, read rects[block base + slot]
    uint32_t slot;                 // record slot in the 256-splat block
    BinRect rect;
};

constexpr uint32_t BIN_WORD_NARROW_TILES = 256;            // the narrow word's origin fields: tile coordinates 0 .. 255
constexpr uint32_t BIN_WORD_MAX_SPAN = 14;                 // largest x1 - x0 / y1 - y0 a direct narrow word holds
constexpr uint32_t BIN_WORD_SPECIAL = 15u << 16;           // x span code 15
constexpr uint32_t BIN_WORD_INVISIBLE = 0x00FF0000u;       // x span 15, y span 15

GS_BIN_WORD_FN BinWordWide bin_word_pack_wide(bool visible, uint32_t slot_in_block, BinRect r) {
    BinWordWide w = {0u, 0u};
    if (!visible) return w;
    w.x = (r.lo & 0xFFFFu) | ((r.lo >> 16) << 12) | (slot_in_block << 24);
    w.y = (r.hi & 0xFFFFu) | ((r.hi >> 16) << 12) | (1u << 24);
    return w;
}
GS_BIN_WORD_FN BinWordOut bin_word_unpack_wide(BinWordWide w) {
    BinWordOut o;
    o.visible = ((w.y >> 24) & 1u) != 0u;
    o.escape = false;
    o.slot = w.x >> 24;
    o.rect.lo = (w.x & 0xFFFu) | (((w.x >> 12) & 0xFFFu) << 16);
    o.rect.hi = (w.y & 0xFFFu) | (((w.y >> 12) & 0xFFFu) << 16);
    return o;
}

GS_BIN_WORD_FN uint32_t bin_word_pack_narrow(bool visible, uint32_t slot_in_block, BinRect r) {
    if (!visible) return BIN_WORD_INVISIBLE;
    const uint32_t span = r.hi - r.lo;                     // (x1 - x0) | (y1 - y0) << 16: x1 >= x0 and y1 >= y0, so no borrow
    // every coordinate <= 255 and both spans <= 14 (x1 <= 255 and y1 <= 255 bound the origins too)
    const bool direct = ((r.hi & 0xFF00FF00u) | (r.lo & 0xFF00FF00u)) == 0u && (span & 0xFFFFu) <= BIN_WORD_MAX_SPAN && (span >> 16) <= BIN_WORD_MAX_SPAN;
    if (!direct) return BIN_WORD_SPECIAL | (slot_in_block << 24);
    return (r.lo & 0xFFu) | ((r.lo >> 16) << 8) | ((span & 0xFu) << 16) | ((span >> 16) << 20) | (slot_in_block << 24);
}
GS_BIN_WORD_FN BinWordOut bin_word_unpack_narrow(uint32_t w) {
    BinWordOut o;
    o.visible = (w & BIN_WORD_INVISIBLE) != BIN_WORD_INVISIBLE;
    o.escape = o.visible && (w & BIN_WORD_SPECIAL) == BIN_WORD_SPECIAL;
    o.slot = w >> 24;
    o.rect.lo = (w & 0xFFu) | (((w >> 8) & 0xFFu) << 16);
    o.rect.hi = o.rect.lo + (((w >> 16) & 0xFu) | (((w >> 20) & 0xFu) << 16));   // (<= 255 + 14 per field: no carry between them)
    return o;
}
