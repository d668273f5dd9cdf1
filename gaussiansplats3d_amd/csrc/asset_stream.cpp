// asset_stream.cpp — see asset_stream.hpp.  Host only.
#include "asset_stream.hpp"

const char* AssetStream::admit(uint64_t bytes) const {
    if (failed) return "the stream refused an earlier append: it takes no more";
    if (complete) return "the stream is complete: the final append was accepted";
    if (bounded && bytes > expected_bytes - bytes_received) return "more bytes than expected_bytes";
    if (bytes > ~(uint64_t)0 - bytes_received) return "the byte count overflows 64 bits";
    return nullptr;
}

uint32_t stream_ready_splats(const std::vector<StreamRun>& runs, uint64_t received, uint32_t limit) {
    uint32_t ready = 0;
    for (const StreamRun& r : runs) {
        if (r.first != ready) break;                                   // a prefix: a run counts only behind a complete one
        if (received < r.gate || received < r.rows_off) break;
        uint64_t rows = r.stride ? (received - r.rows_off) / r.stride : r.count;
        if (rows > r.count) rows = r.count;
        ready += (uint32_t)rows;
        if (rows < r.count) break;
    }
    return ready < limit ? ready : limit;
}

void AssetStream::advance(uint64_t received) {
    bytes_received = received;
    const uint32_t ready = stream_ready_splats(runs, received, splat_limit);
    if (ready > splats_ready) splats_ready = ready;
}

void AssetStream::finish(uint64_t received, uint32_t splat_count) {
    bytes_received = received;
    complete = true;
    header_ready = true;
    splat_limit = splat_count;
    splats_ready = splat_count;
}
