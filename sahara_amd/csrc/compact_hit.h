// compact_hit.h — the host's decoder of compact hit records (hits.hip
// kCompactHits; include/sahara_hip.h sahara_hit_blocks), written once for the
// library's expander (ctx.h) and the command line's writers. Host only; the
// device keeps its own (decodeKey, kExpandRecs, align.hip).
//
// A record v holds the hit's qid relative to its block's first, its position
// in the concatenated text and its errors. The text position names the record
// (the last start at or below it) and the position within it.
#pragma once
#include <algorithm>
#include <cstdint>

namespace sahara_compact {

inline uint64_t qidOf(uint64_t v) { return v >> 36; }  // add the block's block_qid0
inline uint64_t textOf(uint64_t v) { return (v >> 4) & 0xFFFFFFFFull; }
inline uint32_t errOf(uint64_t v) { return (uint32_t)(v & 15u); }

// Text position -> (seq, pos) over `n` ascending starts, starts[0] == 0. The
// last start's record has no end: with the text length as a last start
// (rec_starts' n_records + 1 entries) no valid position reaches it. Hits come
// sorted by (qid, seq_id, pos), so mostly the current record [lo, hi) serves.
struct RecordCursor {
    const uint64_t* starts;
    uint64_t n;
    uint64_t seq = 0, lo = 1, hi = 0;  // the current record's [start, next start): empty
    RecordCursor(const uint64_t* s, uint64_t nStarts) : starts(s), n(nStarts) {}
    uint64_t seek(uint64_t g) {  // moves to g's record, returns g's position in it
        if (g < lo || g >= hi) {
            seq = (uint64_t)(std::upper_bound(starts, starts + n, g) - starts) - 1;
            lo = starts[seq];
            hi = seq + 1 < n ? starts[seq + 1] : UINT64_MAX;
        }
        return g - lo;
    }
};

// Hit index -> its block's first qid: block b holds the hits up to
// block_end[b], an empty one repeats its predecessor's end. Starts at hit k0;
// the hits asked for ascend and lie below block_end[n_blocks - 1].
struct BlockCursor {
    const uint64_t *end, *qid0;
    uint64_t blk;
    BlockCursor(const uint64_t* blockEnd, const uint64_t* blockQid0, uint64_t nBlocks, uint64_t k0)
        : end(blockEnd), qid0(blockQid0), blk((uint64_t)(std::upper_bound(blockEnd, blockEnd + nBlocks, k0) - blockEnd)) {}
    uint64_t qid0Of(uint64_t k) {
        while (k >= end[blk]) ++blk;
        return qid0[blk];
    }
};

}  // namespace sahara_compact
