// rescue_core.h — the pure pieces of the mate rescue (docs/semantics.md "Mate
// rescue"), written once for the kernels (rescue.hip) and for host code
// (tests/rescue_core_check.cpp builds this header alone, no HIP): the window
// of starts a record's missing mate is looked for in, whether a record of the
// sorted batch is an anchor beside its neighbour, and the order of two
// (errors, start) results.
#pragma once
#include <cstdint>

#include "pairs_core.h"

namespace sahara {

// One anchor's scan is at most this many starts: 64 rounds of a wave (a
// policy, SAHARA_RESCUE_MAX_WINDOW in the ABI; a call whose dmax - dmin
// reaches it is refused).
constexpr uint32_t kRescueMaxWindow = 4096;

// The starts [lo, hi] on the hit's own record at which its partner is looked
// for: the pair rule's range (pairRange), clipped to the record's symbols
// [0, recLen). Empty where the range is, or where it begins past the record.
struct RescueWindow {
    bool any;
    uint64_t lo, hi;
};
SAHARA_HD RescueWindow rescueWindow(uint64_t qid, uint64_t pos, uint64_t dmin, uint64_t dmax, uint64_t recLen) {
    const PairRange r = pairRange(qid, pos, dmin, dmax);
    if (!r.any || recLen == 0 || r.lo > recLen - 1) return {false, 0, 0};
    return {true, r.lo, r.hi < recLen - 1 ? r.hi : recLen - 1};
}

// Record i of the sorted batch is an anchor iff it is the first record of its
// (qid, seq, pos) (i == 0, or the record before it differs in one of them),
// the pair rule keeps it not (hasMate: pairKeeps over the batch), and its
// window is not empty.
SAHARA_HD bool rescueIsAnchor(bool isFirst, uint64_t prevQid, uint32_t prevSeq, uint64_t prevPos, uint64_t qid,
                              uint32_t seq, uint64_t pos, bool hasMate, uint64_t dmin, uint64_t dmax, uint64_t recLen) {
    if (hasMate) return false;
    if (!isFirst && prevQid == qid && prevSeq == seq && prevPos == pos) return false;
    return rescueWindow(qid, pos, dmin, dmax, recLen).any;
}

// A scan's result as one word that orders by (errors, start): the least
// errors, ties to the smaller start. at: the start's index in the window,
// below kRescueMaxWindow. kRescueNone: nothing within the bound, above all.
constexpr uint32_t kRescueNone = 0xFFFFFFFFu;
SAHARA_HD uint32_t rescueKey(uint32_t err, uint32_t at) { return err << 16 | at; }
SAHARA_HD uint32_t rescueKeyErr(uint32_t key) { return key >> 16; }
SAHARA_HD uint32_t rescueKeyAt(uint32_t key) { return key & 0xFFFFu; }
SAHARA_HD uint32_t rescueBest(uint32_t a, uint32_t b) { return a < b ? a : b; }

}  // namespace sahara
