// loci_core.h — the two pure functions of the loci stage (docs/semantics.md
// "Loci"), written once for the kernels (loci.hip) and for host code
// (tests/loci_core_check.cpp builds this header alone, no HIP): whether a
// record of the canonically sorted hits starts a new locus, and the key whose
// minimum over a locus names its representative.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SAHARA_HD __host__ __device__ __forceinline__
#else
#define SAHARA_HD inline
#endif

namespace sahara {

// Record i > 0 of the sorted hits against record i - 1 (qid, seq_id, pos of
// each; record 0 is always a head): another query, another record of the
// text, or more than `window` symbols further on. The records are sorted, so
// within one (qid, seq_id) pos >= prevPos, and record i - 1 sits at the same
// position or at the previous distinct one: comparing neighbours is exact.
SAHARA_HD bool lociHead(uint64_t prevQid, uint32_t prevSeq, uint64_t prevPos, uint64_t qid, uint32_t seq, uint64_t pos,
                        uint32_t window) {
    return qid != prevQid || seq != prevSeq || pos - prevPos > window;
}

// The representative of a locus is its record with the least (err, index in
// canonical order): least err, ties to the smaller pos, and among duplicates
// at one position the least err sorts first anyway. One 64-bit minimum finds
// it; a batch holds fewer than 2^32 records.
SAHARA_HD uint64_t lociKey(uint32_t err, uint32_t index) { return ((uint64_t)err << 32) | index; }
SAHARA_HD uint32_t lociKeyIndex(uint64_t key) { return (uint32_t)(key & 0xFFFFFFFFull); }
constexpr uint64_t kLociNoKey = ~0ull;  // above every key: what the per-locus minima start from

}  // namespace sahara
