// pairs_core.h — the pure pieces of the pair stage (docs/semantics.md
// "Pairs"), written once for the kernels (pairs.hip) and for host code
// (tests/pairs_core_check.cpp builds this header alone, no HIP): the partner
// query of a hit, the position range its mates lie in, the order of a record
// against a search key, and whether the record a lower bound found is a mate.
#pragma once
#include <cstdint>

#ifndef SAHARA_HD
#if defined(__HIPCC__)
#define SAHARA_HD __host__ __device__ __forceinline__
#else
#define SAHARA_HD inline
#endif
#endif

namespace sahara {

// Pair p owns the qids 4p (mate A), 4p + 1 (its reverse complement), 4p + 2
// (mate B) and 4p + 3 (rc B): A goes with rc B, B with rc A.
SAHARA_HD uint64_t pairPartner(uint64_t qid) { return qid ^ 3ull; }

// The distances b - a (forward mate at a, reverse mate at b) of a concordant
// pair: the fragment b + len - a lies in [max(minFrag, len), maxFrag].
// Callers refuse maxFrag < len before anything runs.
struct PairDist {
    uint64_t dmin, dmax;
};
SAHARA_HD PairDist pairDist(uint32_t len, uint32_t minFrag, uint32_t maxFrag) {
    const uint64_t least = minFrag > len ? minFrag : len;
    return {least - len, (uint64_t)maxFrag - len};
}

// The positions [lo, hi] at which a hit of `qid` at `pos` has its mates (on
// its own record, under its partner qid). An even qid is the forward mate:
// its mates lie dmin .. dmax to the right (the sum saturates). An odd qid is
// the reverse mate: they lie dmax .. dmin to the left, clipped at 0 before
// the subtraction; none if pos < dmin.
struct PairRange {
    bool any;
    uint64_t lo, hi;
};
SAHARA_HD PairRange pairRange(uint64_t qid, uint64_t pos, uint64_t dmin, uint64_t dmax) {
    if ((qid & 1ull) == 0) {
        const uint64_t room = ~0ull - pos;
        if (dmin > room) return {false, 0, 0};
        return {true, pos + dmin, dmax > room ? ~0ull : pos + dmax};
    }
    if (pos < dmin) return {false, 0, 0};
    return {true, pos > dmax ? pos - dmax : 0, pos - dmin};
}

// A record's (qid, seq_id, pos) against a key: < 0 below it, 0 equal, > 0 above
// (the canonical order's first three fields; err plays no part in the rule).
SAHARA_HD int pairCompare(uint64_t qid, uint32_t seq, uint64_t pos, uint64_t kQid, uint32_t kSeq, uint64_t kPos) {
    if (qid != kQid) return qid < kQid ? -1 : 1;
    if (seq != kSeq) return seq < kSeq ? -1 : 1;
    if (pos != kPos) return pos < kPos ? -1 : 1;
    return 0;
}

// The first record not below (partner, seq, lo) is a mate iff it has that qid
// and that record and lies at or below hi: the records are sorted, so if this
// one lies past hi, so does every later one of the partner on this record.
SAHARA_HD bool pairIsMate(uint64_t qid, uint32_t seq, uint64_t pos, uint64_t partner, uint32_t kSeq, uint64_t hi) {
    return qid == partner && seq == kSeq && pos <= hi;
}

// The whole decision for record i of the n sorted records, over any accessor
// `at(j)` that returns a record with qid, seq_id and pos: the lower bound of
// the key within [first, last) and the mate test. first / last: any range
// that holds every record of the partner qid (the whole batch does).
template <typename At>
SAHARA_HD bool pairKeeps(const At& at, uint64_t qid, uint32_t seq, uint64_t pos, uint64_t dmin, uint64_t dmax,
                         uint64_t first, uint64_t last) {
    const PairRange r = pairRange(qid, pos, dmin, dmax);
    if (!r.any) return false;
    const uint64_t partner = pairPartner(qid);
    uint64_t lo = first, hi = last;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const auto y = at(mid);
        if (pairCompare(y.qid, y.seq_id, y.pos, partner, seq, r.lo) < 0) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= last) return false;
    const auto y = at(lo);
    return pairIsMate(y.qid, y.seq_id, y.pos, partner, seq, r.hi);
}

}  // namespace sahara
