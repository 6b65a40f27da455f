// pair_links_core.h — the pure pieces of the pair stage's links
// (docs/semantics.md "Pair links"), written once for the kernels (pairs.hip)
// and for host code (tests/pair_links_core_check.cpp builds this header alone,
// no HIP): the first record of a mate range that has the range's least err,
// the key that orders a pair's candidates for its primary record, and a
// pair's MAPQ.
#pragma once
#include <cstdint>

#include "best_pairs_core.h"

namespace sahara {

// The smallest index in [lb, ub) whose err is minErr; ub if there is none.
// errAt / blockAt as in bestRangeMin, but read in index order: the partial
// block at the left end record by record, then the whole blocks by their
// minima (the first that holds minErr is scanned, and holds it), then the
// partial block at the right end. At most 126 + 64 + (ub - lb) / 64 reads.
template <typename ErrAt, typename BlockAt>
SAHARA_HD uint64_t bestRangeArgMin(const ErrAt& errAt, const BlockAt& blockAt, uint64_t lb, uint64_t ub,
                                   uint32_t minErr) {
    if (lb >= ub) return ub;
    const uint64_t b0 = (lb + kBestBlock - 1) / kBestBlock, b1 = ub / kBestBlock;  // the whole blocks [b0, b1)
    if (b0 >= b1) {
        for (uint64_t j = lb; j < ub; ++j)
            if (errAt(j) == minErr) return j;
        return ub;
    }
    for (uint64_t j = lb; j < b0 * kBestBlock; ++j)
        if (errAt(j) == minErr) return j;
    for (uint64_t b = b0; b < b1; ++b) {
        if (blockAt(b) != minErr) continue;
        for (uint64_t j = b * kBestBlock; j < (b + 1) * kBestBlock; ++j)
            if (errAt(j) == minErr) return j;
    }
    for (uint64_t j = b1 * kBestBlock; j < ub; ++j)
        if (errAt(j) == minErr) return j;
    return ub;
}

// A pair's primary even-qid record is the kept one with the least (m, index):
// the least of these keys. kLinkNoKey: no candidate.
constexpr unsigned long long kLinkNoKey = ~0ull;
SAHARA_HD unsigned long long pairPrimaryKey(uint32_t m, uint32_t index) {
    return ((unsigned long long)m << 32) | index;
}
SAHARA_HD uint32_t pairPrimaryIndex(unsigned long long key) { return (uint32_t)(key & 0xFFFFFFFFull); }

// The pair's MAPQ (a policy of this build): best = s1, next = the least score
// above it (kBestNone: none), nBest = the larger of the pair's kept even-qid
// and kept odd-qid records with m == s1. Three or more best placements: 0;
// two: 1; one: 10 per error that the next placement costs more, 60 at the most
// and where there is no next. A pair that keeps nothing has none: 0.
constexpr uint32_t kMapqMaxGap = 6;
SAHARA_HD uint32_t pairMapq(uint32_t best, uint32_t next, uint32_t nBest) {
    if (best >= kBestNone || nBest == 0 || nBest >= 3) return 0;
    if (nBest == 2) return 1;
    uint32_t gap = kMapqMaxGap;
    if (next < kBestNone) gap = next > best ? next - best : 0u;
    return 10u * (gap < kMapqMaxGap ? gap : kMapqMaxGap);
}

constexpr uint8_t kLinkPrimary = 1;  // sahara_pair_link.flags, bit 0

}  // namespace sahara
