// best_pairs_core.h — the pure pieces of the pair stage's best mode
// (docs/semantics.md "Best pairs"), written once for the kernels (pairs.hip)
// and for host code (tests/best_pairs_core_check.cpp builds this header alone,
// no HIP): the index range a record's mates lie in, the least err of such a
// range from the per-block minima, and whether a record is kept.
#pragma once
#include <cstdint>

#include "pairs_core.h"

namespace sahara {

// A score that has no value (a record without a mate, a pair that keeps
// nothing): above every sum of two error counts (each below 16).
constexpr uint32_t kBestNone = 255;
constexpr uint32_t kBestMaxDelta = 30;  // the largest difference of two scores
constexpr uint64_t kBestBlock = 64;     // records per block minimum: one wave's

// The first record of [first, last) that is not below (above, if `past`) the
// key (qid, seq, pos) in the canonical order's first three fields.
template <typename At>
SAHARA_HD uint64_t bestBound(const At& at, uint64_t kQid, uint32_t kSeq, uint64_t kPos, bool past, uint64_t first,
                             uint64_t last) {
    uint64_t lo = first, hi = last;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const auto y = at(mid);
        const int c = pairCompare(y.qid, y.seq_id, y.pos, kQid, kSeq, kPos);
        if (c < 0 || (past && c == 0)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The first record of [from, last) above the key, looked for from `from` on in
// steps that double and then by bestBound between the last two probes: a range
// of r records costs some 2 log2(r + 2) probes, close to `from`, where a bound
// over the whole segment costs log2 of that whatever r is. Most ranges hold a
// handful of records.
template <typename At>
SAHARA_HD uint64_t bestBoundNear(const At& at, uint64_t kQid, uint32_t kSeq, uint64_t kPos, uint64_t from,
                                 uint64_t last) {
    uint64_t lo = from, hi = last, step = 1;
    while (lo < hi) {
        const uint64_t probe = hi - lo > step ? lo + step - 1 : hi - 1;
        const auto y = at(probe);
        if (pairCompare(y.qid, y.seq_id, y.pos, kQid, kSeq, kPos) > 0) {
            hi = probe;
            break;
        }
        lo = probe + 1;
        step <<= 1;
    }
    return bestBound(at, kQid, kSeq, kPos, true, lo, hi);
}

// R(i): the records [lb, ub) of the partner of `qid` on record `seq` whose pos
// lies in pairRange(qid, pos, dmin, dmax); lb == ub iff the pair rule drops
// the record. first / last as in pairKeeps: any range that holds every record
// of the partner qid.
struct BestRange {
    uint64_t lb, ub;
};
template <typename At>
SAHARA_HD BestRange bestMateRange(const At& at, uint64_t qid, uint32_t seq, uint64_t pos, uint64_t dmin, uint64_t dmax,
                                  uint64_t first, uint64_t last) {
    const PairRange r = pairRange(qid, pos, dmin, dmax);
    if (!r.any) return {first, first};
    const uint64_t partner = pairPartner(qid);
    const uint64_t lb = bestBound(at, partner, seq, r.lo, false, first, last);
    return {lb, bestBoundNear(at, partner, seq, r.hi, lb, last)};
}

// The least err of the records [lb, ub), kBestNone if there are none. errAt(j):
// record j's err; blockAt(b): the least err of the records [64 b, 64 b + 64).
// The partial blocks at both ends are read record by record (at most 126
// reads, or the whole range if it holds no whole block) and the whole blocks
// between them by their minima, so the work is 126 + (ub - lb) / 64 reads at
// the most; it ends at the first 0, which nothing undercuts.
template <typename ErrAt, typename BlockAt>
SAHARA_HD uint32_t bestRangeMin(const ErrAt& errAt, const BlockAt& blockAt, uint64_t lb, uint64_t ub) {
    uint32_t m = kBestNone;
    if (lb >= ub) return m;
    const uint64_t b0 = (lb + kBestBlock - 1) / kBestBlock, b1 = ub / kBestBlock;  // the whole blocks [b0, b1)
    if (b0 >= b1) {
        for (uint64_t j = lb; j < ub && m; ++j) {
            const uint32_t e = errAt(j);
            m = e < m ? e : m;
        }
        return m;
    }
    for (uint64_t j = lb; j < b0 * kBestBlock && m; ++j) {
        const uint32_t e = errAt(j);
        m = e < m ? e : m;
    }
    for (uint64_t j = b1 * kBestBlock; j < ub && m; ++j) {
        const uint32_t e = errAt(j);
        m = e < m ? e : m;
    }
    for (uint64_t b = b0; b < b1 && m; ++b) {
        const uint32_t e = blockAt(b);
        m = e < m ? e : m;
    }
    return m;
}

// m(i) = e(i) + the least err of R(i); no value without a mate
SAHARA_HD uint32_t bestScore(uint32_t err, uint32_t mateMin) { return mateMin == kBestNone ? kBestNone : err + mateMin; }

// Record i is kept iff it is the first of its (qid, seq, pos), m(i) has a
// value and m(i) <= s1(P) + delta (best: s1 of its pair; it has a value
// whenever some m of the pair has).
SAHARA_HD bool bestKeeps(bool firstOfPos, uint32_t m, uint32_t best, uint32_t delta) {
    return firstOfPos && m != kBestNone && m <= best + delta;
}

}  // namespace sahara
