"""The binner's look-up word (csrc/bin_word.hpp) and which of its two widths a draw uses (csrc/draw_plan.cpp, narrow_bin_word),
through the library's pure-host debug entry gs_debug_bin_word: no GPU.  The entry packs one splat position into the 4-byte and
into the 8-byte word and unpacks both with the functions k_project and k_bin_count are built from.  What must hold: a visible
position comes back with the rect and the slot it went in with, or - a span above 14 tiles, a coordinate above 255 - as an
escape that still carries the slot; nothing visible encodes to the word that means "not visible"; and the 8-byte word, which the
4-byte one replaces, says the same."""
import ctypes as C
import itertools

import pytest

import gaussiansplats3d_amd as g

INVISIBLE = 0x00FF0000


class WordIn(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("tiles_x", "tiles_y", "no_compact_bin_word", "visible", "slot", "x0", "y0", "x1", "y1")]


class WordOut(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("narrow", "word", "visible", "escape", "slot", "x0", "y0", "x1", "y1", "wide_lo", "wide_hi",
                                          "wide_visible", "wide_slot", "wide_x0", "wide_y0", "wide_x1", "wide_y1")]


def _entry():
    fn = g.load().gs_debug_bin_word
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(WordIn), C.POINTER(WordOut)]
    return fn


def word(visible=1, slot=0, rect=(0, 0, 0, 0), tiles=(120, 68), switch=0):
    s, out = WordIn(tiles[0], tiles[1], switch, visible, slot, *rect), WordOut()
    assert _entry()(C.byref(s), C.byref(out)) == 0
    return out


def rect_of(origin_x, origin_y, span_x, span_y):
    return (origin_x, origin_y, origin_x + span_x, origin_y + span_y)


DIRECT_SPANS, ESCAPE_SPANS = (0, 1, 14), (15, 119)


def check_wide(out, slot, rect):
    assert out.wide_visible == 1 and out.wide_slot == slot
    assert (out.wide_x0, out.wide_y0, out.wide_x1, out.wide_y1) == rect


def test_null_arguments_are_refused():
    assert _entry()(None, None) == -1


def fits(rect):
    """What the 4-byte word holds directly: every coordinate <= 255, both spans <= 14."""
    return max(rect) <= 255 and rect[2] - rect[0] <= 14 and rect[3] - rect[1] <= 14


@pytest.mark.parametrize("span_x,span_y", list(itertools.product(DIRECT_SPANS, DIRECT_SPANS)))
def test_direct_words_return_rect_and_slot(span_x, span_y):
    """Every slot; the origin at 0, at 255 (direct only while the far edge stays at 255: a single tile in that direction) and where the far
    edge is 255."""
    words = {}
    for ox, oy in itertools.product((0, 255 - span_x, 255), (0, 255 - span_y, 255)):
        rect = rect_of(ox, oy, span_x, span_y)
        for slot in range(256):
            out = word(slot=slot, rect=rect, tiles=(4096, 4096))
            assert (out.visible, out.slot) == (1, slot), (rect, slot, hex(out.word))
            assert out.escape == (0 if fits(rect) else 1), (rect, slot, hex(out.word))
            if fits(rect):
                assert (out.x0, out.y0, out.x1, out.y1) == rect, (rect, slot, hex(out.word))
                assert words.setdefault(out.word, (rect, slot)) == (rect, slot)                 # one word, one meaning
            assert out.word & INVISIBLE != INVISIBLE
            check_wide(out, slot, rect)
    assert len(words) >= 256


@pytest.mark.parametrize("span", ESCAPE_SPANS)
def test_wide_spans_escape_with_their_slot(span):
    for rect in (rect_of(0, 0, span, 0), rect_of(0, 0, 0, span), rect_of(3, 5, span, span), rect_of(0, 0, span, 14), rect_of(0, 0, 14, span)):
        for slot in range(256):
            out = word(slot=slot, rect=rect)
            assert (out.visible, out.escape, out.slot) == (1, 1, slot), (rect, slot, hex(out.word))
            assert out.word & INVISIBLE != INVISIBLE
            check_wide(out, slot, rect)                                                         # the 8-byte word holds it


def test_origin_256_escapes():
    for rect in ((256, 0, 256, 0), (0, 256, 0, 256), (256, 256, 257, 257), (4095, 4095, 4095, 4095)):
        for slot in (0, 1, 255):
            out = word(slot=slot, rect=rect, tiles=(4096, 4096))
            assert (out.visible, out.escape, out.slot) == (1, 1, slot), (rect, slot, hex(out.word))
            check_wide(out, slot, rect)


def test_no_visible_input_makes_the_invisible_word():
    out = word(visible=0, slot=0, rect=(0, 0, 0, 0))
    assert out.word == INVISIBLE and (out.visible, out.escape) == (0, 0)
    assert (out.wide_lo, out.wide_hi, out.wide_visible) == (0, 0, 0)
    # whatever an invisible position carries, it stays invisible
    assert word(visible=0, slot=255, rect=(255, 255, 255, 255)).visible == 0
    # ... and no visible one is mistaken for it: every slot, every pair of span codes 0 .. 16 (15 is the reserved code, 16 wraps to
    # 0 in a 4-bit field) at both origins, and the coordinates whose low bits look like the reserved codes
    rects = [rect_of(o, o, sx, sy) for o in (0, 240) for sx in range(17) for sy in range(17)]
    rects += [(15, 15, 15, 15), (255, 255, 255, 255), (0, 0, 255, 255), (255, 0, 255, 255), (0, 0, 0xFFF, 0xFFF), (0xF0F, 0xF0F, 0xFFF, 0xFFF)]
    for rect in rects:
        for slot in (0, 15, 240, 255):
            out = word(slot=slot, rect=rect, tiles=(4096, 4096))
            assert out.visible == 1 and out.word != INVISIBLE and out.word & INVISIBLE != INVISIBLE, (rect, slot, hex(out.word))
            assert out.slot == slot
            if not out.escape:
                assert (out.x0, out.y0, out.x1, out.y1) == rect
            else:
                assert max(rect) > 255 or rect[2] - rect[0] > 14 or rect[3] - rect[1] > 14, rect   # nothing escapes that fits


def test_which_word_a_draw_uses():
    assert word(tiles=(256, 256)).narrow == 1
    assert word(tiles=(120, 68)).narrow == 1 and word(tiles=(240, 135)).narrow == 1              # 1080p, 4K
    assert word(tiles=(257, 1)).narrow == 0
    assert word(tiles=(1, 257)).narrow == 0
    assert word(tiles=(480, 270)).narrow == 0                                                    # 8K
    for tiles in ((256, 256), (120, 68), (1, 1)):
        assert word(tiles=tiles, switch=1).narrow == 0                                           # $GSPLAT_NO_COMPACT_BIN_WORD
