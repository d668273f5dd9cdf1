// asset_stream.hpp — the state of a streamed asset (gs_asset_open_stream / gs_asset_append: assets.hip): which appends are
// taken, and how many splats of the file's numbering are ready for an upload after how many bytes.  Host only: no HIP, no
// gs_asset, no context.  The format readers (assets.hip) say, once a header is in, where the rows lie (StreamRun); everything
// else here is byte counting.  tests/test_asset_stream.py holds it to a model of each format through gs_asset_get_stream_info;
// tests/tools/asset_stream_fuzz.cpp is the stand-alone program for a sanitizer run.
//
// Two rules.  M: when the final append is accepted the stream is the asset gs_asset_open returns for the concatenated bytes.
// P: at any moment the ready splats are a prefix [0, splats_ready) of the whole file's numbering, and splats_ready never decreases.
// A splat is ready when every byte its decode reads has arrived.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// What a header reader answers when the bytes it was given end before the header does and more may come (a positive status,
// never handed to a caller of the C ABI: the whole-file reader turns it into its refusal, the stream waits).
constexpr int STREAM_NEED_MORE = 100;
// "the file's size is not known yet": a reader given this checks nothing against the end of the file
constexpr size_t STREAM_SIZE_UNKNOWN = ~(size_t)0;

// Splats [first, first + count) become ready row by row: nothing before `gate` bytes have arrived (a table every row reads: the
// chunk element of a compressed PLY, a .ksplat section's bucket block), then splat first + k with the byte rows_off + stride * (k + 1).
// The rows a splat reads in more than one element (compressed PLY with SH) are counted by the element that arrives last.
struct StreamRun {
    uint64_t gate, rows_off;
    uint32_t stride, first, count;
};

struct AssetStream {
    uint32_t format = 0, max_sh_degree = 0;
    uint64_t expected_bytes = 0;           // 0: not known (refused for .splat, whose splat count comes from it)
    bool bounded = false;                  // bytes beyond expected_bytes are refused (.splat)
    uint64_t bytes_received = 0;
    bool header_ready = false, complete = false, failed = false;
    uint32_t splats_ready = 0;
    uint32_t splat_limit = 0;              // the header's splat count: what the runs are capped at
    std::vector<StreamRun> runs;           // in file order, each beginning where the one before ends
    std::vector<uint8_t> raw;              // .spz: the gzip member as it arrives (inflated into the asset at the final append)

    // May an append of `bytes` be looked at?  nullptr, or why not (then nothing is consumed and the state stays)
    const char* admit(uint64_t bytes) const;
    // The readers have replaced `runs` for the bytes now present: the ready prefix, never smaller than before
    void advance(uint64_t received);
    // An append was refused: no further append is taken; what is ready stays ready
    void refuse() { failed = true; }
    // The final append was accepted: all `splat_count` splats are ready
    void finish(uint64_t received, uint32_t splat_count);
};

// the prefix of [0, limit) that `runs` make ready after `received` bytes
uint32_t stream_ready_splats(const std::vector<StreamRun>& runs, uint64_t received, uint32_t limit);
