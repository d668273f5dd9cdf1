"""Host model of the binner's entry lists (gaussiansplats3d_amd/csrc/tile_bin.hip: k_bin_count, k_bin_emit and the
entry sort): plain numpy integers, none of the kernels' slices, batches, offsets or radix passes.

The contract it states:
  The list of a list bin holds exactly the visible splats of the render list whose tile rect touches that bin, one entry per
  occurrence in the render list, in near -> far order - which is the render list walked from its end.

Read next to the kernels:
  p = R-1 ... 0                      -> the walk (bin_count_slice: p = R - 1 - q)
  idx >= n, invisible                -> dropped (keep[k]; "entries beyond the uploaded splats draw nothing")
  rect_to_bins(r, list_shift)        -> every field of {x0 | y0 << 16, x1 | y1 << 16} shifted on its own
  bin_emit_batch                     -> one (list bin, record slot) pair per bin of the rect
  the stable entry sort by bin id    -> a stable argsort by (by - list_row_begin) * lists_x + bx
  the published [begin, end)         -> run starts / ends of the sorted keys; a list nobody touched reads (~0, 0)

The inputs `visible`, `rects` and `slot_of_splat` are the vertex stage's own outputs (gs_mesh_debug_read what = 3 / 1 / 9, in the
caller's numbering): the vertex stage is pinned elsewhere, this model isolates the binner and needs no tolerance.  The binner
gathers the rect from the packed word k_project leaves beside it (12 bits per field); a frame is at most 4096 x 4096 tiles, so
the two hold the same four numbers.
"""
from typing import NamedTuple

import numpy as np

UNTOUCHED = (0xFFFFFFFF, 0)


class Lists(NamedTuple):
    ranges: np.ndarray       # uint32 [lists, 2]: [begin, end) into `entries`, UNTOUCHED where a list is empty
    entries: np.ndarray      # uint32 [D]: record slots, list after list, each near -> far
    walk: np.ndarray         # int64 [V]: the caller's splat index of every surviving list position, near -> far
    walk_q: np.ndarray       # int64 [V]: how far into the walk each of them sits (q = R - 1 - p of its list position p)
    runs: np.ndarray         # int64 [V]: list bins (= entries) of each of them
    tiles16: int             # sum over them of the 16-px tiles their rect covers (gs_render_stats.tiles16)
    entry_walk: np.ndarray   # int64 [D]: per entry, the position in `walk` it came from


def rect_fields(rects, shift=0):
    r = np.asarray(rects, dtype=np.uint32).reshape(-1, 2).astype(np.int64)
    return (r[:, 0] & 0xFFFF) >> shift, (r[:, 0] >> 16) >> shift, (r[:, 1] & 0xFFFF) >> shift, (r[:, 1] >> 16) >> shift


def bins_of(rects, shift):
    """List bins (shift = list_shift) or 16-px tiles (shift = 0) a rect covers; an inverted rect covers none."""
    x0, y0, x1, y1 = rect_fields(rects, shift)
    return np.where((x1 >= x0) & (y1 >= y0), (x1 - x0 + 1) * (y1 - y0 + 1), 0)


def expected_lists(order, render_count, visible, rects, slot_of_splat, list_shift, lists_x, list_row_begin, list_rows):
    visible = np.asarray(visible, dtype=bool)
    slot_of_splat = np.asarray(slot_of_splat, dtype=np.uint32)
    n = visible.shape[0]
    R = int(render_count)
    walk = np.asarray(order, dtype=np.uint32)[:R].astype(np.int64)[::-1]      # p = R-1 ... 0
    assert walk.shape[0] == R, "the render list is shorter than render_count"
    q = np.arange(R, dtype=np.int64)
    q, walk = q[walk < n], walk[walk < n]
    q, walk = q[visible[walk]], walk[visible[walk]]
    r = np.asarray(rects, dtype=np.uint32).reshape(-1, 2)[walk]
    x0, y0, x1, y1 = rect_fields(r, list_shift)
    runs = bins_of(r, list_shift)
    w = np.maximum(x1 - x0 + 1, 1)
    src = np.repeat(np.arange(walk.shape[0], dtype=np.int64), runs)           # the splat of every entry, in walk order
    k = np.arange(src.shape[0], dtype=np.int64) - np.repeat(np.cumsum(runs) - runs, runs)
    bx, by = x0[src] + k % w[src], y0[src] + k // w[src] - int(list_row_begin)
    if src.shape[0] and not ((bx >= 0) & (bx < lists_x) & (by >= 0) & (by < list_rows)).all():
        raise ValueError("a visible splat's rect leaves the list-bin grid of the drawn strip")
    key = by * int(lists_x) + bx
    by_list = np.argsort(key, kind="stable")
    lists = int(lists_x) * int(list_rows)
    counts = np.bincount(key, minlength=lists).astype(np.int64)
    end = np.cumsum(counts)
    ranges = np.empty((lists, 2), dtype=np.uint32)
    ranges[:, 0] = np.where(counts > 0, end - counts, UNTOUCHED[0])
    ranges[:, 1] = np.where(counts > 0, end, UNTOUCHED[1])
    return Lists(ranges, slot_of_splat[walk][src][by_list], walk, q, runs, int(bins_of(r, 0).sum()), src[by_list])
