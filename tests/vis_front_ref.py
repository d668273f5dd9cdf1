"""A plain numpy model of the visibility-culled sort's front ends (csrc/sorter.hip) AS CHUNKED ALGORITHMS: the cut of the list into
workgroup chunks (chunk_grid), the survivor counts per chunk or piece, the exclusive offsets, the compaction turn by turn, the
partial last mask word and the consumption of the mask (copied, then zeroed).  Three front ends:

  stream           k_mask_count + k_cull_front: chunks of whole turns of TURN positions, four waves of WAVE_RUN positions per turn
  lazy             k_mask_derive_count + k_cull_front: the mask derived from the storage-order one first; chunks of whole
                   DERIVE_SUBS x TURN positions, the counts arrive in DERIVE_SUBS pieces per chunk
  compact          k_minmax_count + k_mask_compact: chunks of whole spans of SPAN positions, compacted in iterations of COMPACT_ITER

The constants restate the kernels' (VC_TURN = VC_UNROLL * VC_WAVE_SPAN * 4 waves = 2048 positions).  The model is what the
CPU tier (test_vis_front_ref.py) mutates to prove that the case list of the GPU tier (vis_front_cases.py) is sharp, and where the
single-survivor patterns take their boundary positions from (geometry)."""
import numpy as np

THREADS, WAVES = 256, 4
SPAN = 1024                          # k_minmax_count: positions per workgroup iteration
WAVE_RUN = 512                       # k_cull_front: positions per wave and turn (VC_UNROLL * VC_WAVE_SPAN)
TURN = WAVE_RUN * WAVES              # k_cull_front: positions per workgroup and turn (VC_TURN)
DERIVE_SUBS = 4                      # k_mask_derive_count: workgroups (pieces) per chunk
DERIVE_ROUND = 8 * 64 * WAVES        # ... positions per workgroup and round
COMPACT_ITER = 32 * THREADS          # k_mask_compact: positions per workgroup iteration (one mask word per thread)
COARSE_BLOCKS = 65536                # k_mask_derive_count keeps block_any as bits in LDS up to this many storage blocks
UNWRITTEN = 0xFFFFFFFF               # a slot of the compacted list that no workgroup wrote

FRONTS = ("stream", "lazy", "compact")
UNIT = {"stream": TURN, "lazy": TURN * DERIVE_SUBS, "compact": SPAN}
STEP = {"stream": TURN, "lazy": TURN, "compact": COMPACT_ITER}       # a workgroup's inner loop ("turn")

# what a front end could get wrong without any frame changing (the binner tests visibility again)
MUTATIONS = ("minmax_over_survivors",      # min / max reduced over the survivors instead of every position
             "last_word_not_masked",       # positions at or beyond R in the list's last mask word are counted and emitted
             "before_off_by_one_chunk",    # a chunk's first slot = the survivors of the chunks before the PREVIOUS one
             "turn_parity_reused",         # s_turn single buffered: turn t >= 2 reads the wave counts of turn t - 2
             "mask_not_rezeroed",          # the consumed mask keeps its bits
             "bits_beyond_R_counted")      # the count kernel walks its chunk to the chunk's nominal end, not to R


def chunk_grid(R, unit, T):
    """(workgroups, positions per workgroup) for R > 0 positions: contiguous runs of whole units, at most T = 2 x CUs workgroups."""
    units = (R + unit - 1) // unit
    grid = min(units, T)
    return grid, ((units + grid - 1) // grid) * unit


def geometry(R, T, front):
    """Where the chunked algorithm has its boundaries for a list of R positions: {grid, len, step, chunk_edges, turn_edges (inside
    a chunk, not its begin), third_turn_edges (begin of a chunk's third turn: the double buffer is reused there), last_chunk = [begin,
    end) of the last non-empty chunk, empty_chunks}."""
    grid, ln = chunk_grid(R, UNIT[front], T)
    step = STEP[front]
    begins = np.minimum(np.arange(grid, dtype=np.int64) * ln, R)
    ends = np.minimum(begins + ln, R)
    live = begins < ends
    chunk_edges = [int(b) for b in begins[live] if b > 0]
    turn_edges, third = [], []
    for b, e in zip(begins[live], ends[live]):
        k = np.arange(b + step, e, step)
        turn_edges += [int(v) for v in k]
        if b + 2 * step < e:
            third.append(int(b + 2 * step))
    last = int(np.nonzero(live)[0][-1])
    return {"grid": grid, "len": ln, "step": step, "chunk_edges": chunk_edges, "turn_edges": turn_edges, "third_turn_edges": third,
            "last_chunk": (int(begins[last]), int(ends[last])), "empty_chunks": int((~live).sum())}


def turn_index(R, T, front):
    """Per position of [0, R): the index of its turn inside its chunk."""
    _, ln = chunk_grid(R, UNIT[front], T)
    i = np.arange(R, dtype=np.int64)
    return (i % ln) // STEP[front]


def buckets(keys, lo, hi, precision=16):
    """The reference's bucket of an int32 key for the range [lo, hi] (sorter.cpp; oracle.sort_indexes_numpy)."""
    rng = 1 << precision
    if hi == lo:
        return np.zeros(keys.shape[0], dtype=np.int64)
    range_map = np.float32(rng - 1) / (np.float32(hi) - np.float32(lo))
    diff = ((keys.astype(np.int64) - lo) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return np.clip(np.trunc(diff.astype(np.float32) * range_map).astype(np.int64), 0, rng - 1)


def sort_compacted(listed, keys, lo, hi, precision=16):
    """The radix sort behind the front end: the compacted list by descending bucket, ties in reversed list order."""
    k = np.where(listed < keys.shape[0], keys[np.minimum(listed, keys.shape[0] - 1)], 0).astype(np.int32)
    order = np.argsort(buckets(k, lo, hi, precision), kind="stable")
    return listed[order][::-1]


def derive(vis_storage, pos_of, block_any, R, T, mask):
    """k_mask_derive_count: position i of the identity list is the splat at storage position pos_of[i]; its bit is the vertex
    stage's storage-order bit, gathered only where the storage block has a survivor at all.  Writes the 64-bit words that hold a
    position below R (bits at or beyond R zero) into `mask` (bool per position, a whole number of 64-bit words long), leaves the
    words beyond as they were, and returns the survivor count per piece."""
    grid, ln = chunk_grid(R, UNIT["lazy"], T)
    piece = ln // DERIVE_SUBS
    p = pos_of[:R].astype(np.int64)
    bits = block_any[p >> 8].astype(bool) & vis_storage[p].astype(bool)
    words = (R + 63) // 64
    mask[:words * 64] = False
    mask[:R] = bits
    padded = np.zeros(grid * ln, dtype=np.int64)
    padded[:R] = bits
    return padded.reshape(grid * DERIVE_SUBS, piece).sum(axis=1)


def front_end(front, mask, keys, R, T, mutation=None, precision=16, derived_counts=None):
    """One visibility-culled sort of the identity list [0, R) over `mask` (bool per ORIGINAL splat index, at least R long and a
    whole number of 64-bit words; changed in place as the kernels change the buffer).  keys: the int32 key of every position.
    Returns {list (the sorted list, `kept` long), kept, key_min, key_max, keep_bits (the sorter's copy of the mask, R long)}."""
    assert front in FRONTS and (mutation is None or mutation in MUTATIONS) and R > 0 and mask.shape[0] % 64 == 0
    grid, ln = chunk_grid(R, UNIT[front], T)
    word_end = min((R + 31) // 32 * 32, mask.shape[0])         # the last mask word a workgroup reads ends here
    begins = np.minimum(np.arange(grid, dtype=np.int64) * ln, R)
    # -- the count kernel: set bits per chunk (per piece of a chunk where the mask was derived), the last partial word masked
    counted = np.zeros(grid * ln + 32, dtype=np.int64)
    counted[:R] = mask[:R]
    if mutation == "last_word_not_masked":
        counted[R:word_end] = mask[R:word_end]
    if mutation == "bits_beyond_R_counted":
        reach = min(grid * ln, mask.shape[0])
        counted[R:reach] = mask[R:reach]
    subs = DERIVE_SUBS if front == "lazy" else 1
    pieces = counted[:grid * ln].reshape(grid * subs, ln // subs).sum(axis=1)
    pieces[-1] += counted[grid * ln:].sum()
    if front == "lazy" and derived_counts is not None and mutation is None:
        assert np.array_equal(pieces, derived_counts)           # the derive step counted what it wrote
    counts = pieces.reshape(grid, subs).sum(axis=1)
    kept = int(counts.sum())
    before = np.concatenate([[0], np.cumsum(counts)[:-1]])
    if mutation == "before_off_by_one_chunk":
        before = np.concatenate([[0], before[:-1]])
    # -- min / max
    over = keys[:R][mask[:R]] if mutation == "minmax_over_survivors" else keys[:R]
    lo, hi = (int(over.min()), int(over.max())) if over.size else (0, 0)
    # -- the compaction: what each lane sees of the mask
    seen = np.zeros(grid * ln, dtype=bool)
    seen[:R] = mask[:R]
    if mutation == "last_word_not_masked":
        # k_cull_front looks at nibbles of four positions, k_mask_compact at whole 32-bit words
        reach = min((R + 3) // 4 * 4 if front != "compact" else word_end, grid * ln)
        seen[R:reach] = mask[R:reach]
    slots = np.full(max(kept, int(seen.sum())) + 1, UNWRITTEN, dtype=np.uint32)
    pos = np.arange(grid * ln, dtype=np.int64)
    if front == "compact":
        # a block scan over one word per thread per iteration: ascending inside the chunk
        rank = np.cumsum(seen.reshape(grid, ln), axis=1).reshape(-1) - seen
        slot = np.repeat(before, ln) + rank
    else:
        # turn by turn: the wave's first slot = the workgroup's running slot + the lower waves' survivors of the turn
        turns = ln // TURN
        s4 = seen.reshape(grid, turns, WAVES, WAVE_RUN)
        cnt = s4.sum(axis=3)                                                   # [chunk, turn, wave]
        used = cnt.copy()
        if mutation == "turn_parity_reused" and turns > 2:
            used[:, 2:] = cnt[:, :-2]
        turn_total = used.sum(axis=2)
        out = before[:, None] + np.cumsum(turn_total, axis=1) - turn_total     # running slot at the turn's start
        wave_out = out[:, :, None] + np.cumsum(used, axis=2) - used
        rank = np.cumsum(s4, axis=3) - s4
        slot = (wave_out[:, :, :, None] + rank).reshape(-1)
    w = seen & (slot >= 0) & (slot < slots.shape[0])
    slots[slot[w]] = pos[w].astype(np.uint32)
    # -- the mask is consumed: every word that holds a position below R is copied, then zeroed
    keep_bits = mask[:R].copy()
    if mutation != "mask_not_rezeroed":
        mask[:word_end] = False
    return {"list": sort_compacted(slots[:kept], keys, lo, hi, precision), "kept": kept, "key_min": lo, "key_max": hi,
            "keep_bits": keep_bits}


def same(a, b):
    return (a["kept"] == b["kept"] and a["key_min"] == b["key_min"] and a["key_max"] == b["key_max"] and
            np.array_equal(a["list"], b["list"]) and np.array_equal(a["keep_bits"], b["keep_bits"]))


def storage_order(n, seed=5):
    """A stand-in for the mesh's position map on the host: a fixed pseudo-random permutation (original index -> storage position)."""
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def run_sequence(front, steps, n, keys, T, mutation=None, precision=16):
    """Projections and sorts in turn over one mask buffer, with the flags gs_mesh_project and the sort keep about it (dirty: the
    buffer may hold bits; lazy: the sorter derives the mask; tail_zero: the words the sorter will not write are zero).  steps:
    [(visible bool [n], R)].  A full-frame projection of a `lazy` front end leaves the mask to the sorter; every other one clears a
    dirty buffer and ORs its survivors in.  Returns the result of every sort."""
    mask = np.zeros((n + 63) // 64 * 64, dtype=bool)
    dirty, out = False, []
    pos_of = storage_order(n)
    for vis, R in steps:
        lazy = front == "lazy"
        derived = None
        if lazy:
            tail_zero = not dirty
            vis_storage = np.zeros(n, dtype=bool)
            vis_storage[pos_of] = vis
            block_any = np.zeros((n + 255) // 256 * 256, dtype=bool)
            block_any[:n] = vis_storage
            derived = derive(vis_storage, pos_of, block_any.reshape(-1, 256).any(axis=1), R, T, mask)
        else:
            if dirty:
                mask[:] = False
            mask[:n] |= vis                                    # one atomicOr per survivor
        dirty = True
        out.append(front_end(front, mask, keys, R, T, mutation, precision, derived))
        if R >= n and (not lazy or tail_zero):
            dirty = False
    return out
