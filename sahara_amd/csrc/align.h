// align.h — host-side launch interface of the alignment kernel (align.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sahara_hip.h"

namespace sahara {

// One launch of kAlignHits over a chunk of hit records of one index part.
// The records were checked before (capi_align.cpp): every qid names a pattern,
// every position lies in the text.
struct AlignArgs {
    const uint4* text3;        // the part's text as 3-bit-plane blocks (device_index.h)
    uint32_t text3Bytes;       // its bytes (buffer-load bound; < 4 GiB)
    const uint4* pats3;        // every pattern of the call, patBlocks blocks each, one spare block after the last
    uint32_t patBlocks;
    uint32_t m;
    uint32_t maxErr;           // K <= SAHARA_ALIGN_MAX_ERR
    uint32_t edit;
    uint64_t nHits;            // records of the chunk
    // whole records: the part's record starts (part-local), its first global
    // record and its number of records; a hit of another part is left alone
    const sahara_hit* hits;
    const uint64_t* recStarts;
    uint64_t rec0, nrec;
    // compact records (hits == nullptr): the chunk's 8-B records, its first
    // record's index in the call, and the call's blocks
    const uint64_t* recs;
    uint64_t first;
    const uint64_t* blockEnd;
    const uint64_t* blockQid0;
    uint32_t nBlocks;
    sahara_alignment* out;     // record i of the chunk
};

void launchAlignHits(const AlignArgs& a, hipStream_t st);

}  // namespace sahara
