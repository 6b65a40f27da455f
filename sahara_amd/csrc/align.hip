// align.hip — kAlignHits: the alignment of located hits on the device
// (docs/semantics.md "Alignments"). One lane per hit: the lane
// runs align_core.h's furthest-reaching table against the resident text and
// the call's staged patterns, both 3-bit-plane blocks, and writes one 24-B
// sahara_alignment. A slide along a diagonal is a funnel shift of two
// adjacent blocks of each side, three xors and a count of trailing zeros per
// 32 symbols. The table ((K + 1)(2K + 1) 16-bit entries per lane) lives in
// LDS, lane-interleaved: it is indexed by the row and the diagonal at run
// time, which registers cannot be, and K = 8 would need 153 of them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "align.h"
#include "align_device.h"
#include "device_index.h"

namespace sahara {

namespace {

constexpr uint32_t kAlignBlock = kAlignLanes;  // one wave (align_device.h)

static_assert(sizeof(sahara_alignment) == 24, "sahara_alignment is 24 B");
static_assert(kAlignMaxErr == SAHARA_ALIGN_MAX_ERR && kAlignNone == SAHARA_ALIGN_NONE, "align_core.h mirrors the ABI");

struct PatBlocks {
    const uint4* p;  // the lane's pattern
    __device__ __forceinline__ Planes3 operator()(uint32_t b) const {
        const uint4 v = p[b];
        return {v.x, v.y, v.z};
    }
};

template <bool COMPACT>
__global__ __launch_bounds__(kAlignBlock) void kAlignHits(AlignArgs a) {
    extern __shared__ int16_t alignLds[];
    const uint64_t i = (uint64_t)blockIdx.x * kAlignBlock + threadIdx.x;
    if (i >= a.nHits) return;
    uint64_t qid;
    uint32_t g;
    if (COMPACT) {
        const uint64_t v = a.recs[i], at = a.first + i;
        uint32_t lo = 0, hi = a.nBlocks - 1;  // the first block that ends after record `at`
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.blockEnd[mid] > at) hi = mid; else lo = mid + 1;
        }
        qid = a.blockQid0[lo] + (v >> 36);
        g = (uint32_t)(v >> 4);
    } else {
        const sahara_hit h = a.hits[i];
        if (h.seq_id < a.rec0 || h.seq_id - a.rec0 >= a.nrec) return;  // another part's record
        qid = h.qid;
        g = (uint32_t)(a.recStarts[h.seq_id - a.rec0] + h.pos);
    }
    BufBlocks text{alignBufferOf(a.text3, a.text3Bytes)};
    PatBlocks pat{a.pats3 + qid * a.patBlocks};
    LaneTable L{alignLds + threadIdx.x};
    uint32_t err, refLen;
    uint64_t edLo, edHi;
    alignOne(pat, text, g, a.m, a.maxErr, a.edit != 0, L, err, refLen, edLo, edHi);
    uint2* o = reinterpret_cast<uint2*>(a.out + i);
    o[0] = make_uint2(err, refLen);
    o[1] = make_uint2((uint32_t)edLo, (uint32_t)(edLo >> 32));
    o[2] = make_uint2((uint32_t)edHi, (uint32_t)(edHi >> 32));
}

}  // namespace

void launchAlignHits(const AlignArgs& a, hipStream_t st) {
    if (a.nHits == 0) return;
    const size_t lds = alignTableBytes(a.maxErr, a.edit != 0);
    const uint64_t blocks = (a.nHits + kAlignBlock - 1) / kAlignBlock;
    if (blocks > 0x7FFFFFFFull) throw Error("alignment chunk too large");
    if (a.hits) hipLaunchKernelGGL(kAlignHits<false>, dim3((unsigned)blocks), dim3(kAlignBlock), lds, st, a);
    else        hipLaunchKernelGGL(kAlignHits<true>, dim3((unsigned)blocks), dim3(kAlignBlock), lds, st, a);
    SH_HIP(hipGetLastError());
}

}  // namespace sahara
