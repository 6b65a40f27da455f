// pairs.hip — the pair stage of a batch's chain (docs/semantics.md "Pairs",
// DESIGN.md §3.10): a batch's whole hits, in canonical order after the sort
// (and after the loci stage, if that is on), cut down to the hits that have a
// concordant mate before anything leaves the device (gfx950). Work is per
// hit, as in loci.hip: a query inside a repeat has 10^4..10^5 rows.
//
//   kPairFlags    record i has a mate? one lower bound   -> flag[i]
//   rocPRIM scan  inclusive sum of the flags             -> num[i]; num[rows - 1] = kept (hits.hip scanFlagsCount)
//   kPairGather   the kept records, in order             -> scratch, copied back over the batch (replaceBatch);
//                 the pairs among them                   -> one counter
//
// A pair's four qids lie in one batch (pass_plan.h, granularity 4), so the
// partner's records are all here. The rule's pieces are pairs_core.h's.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "pairs_core.h"
#include "search_device.h"

namespace sahara {
namespace {

struct HitAt {
    const sahara_hit* h;
    __device__ __forceinline__ sahara_hit operator()(uint64_t i) const { return h[i]; }
};

// One lower bound per record, over the partner query's segment
// [qoff[p], qoff[p + 1]) of the batch's per-query offsets (p = partner -
// qidBase): two dependent loads in front, then a handful of levels. (Over the
// whole batch it is some 25 levels: 0.97 ms against 0.59 ms for 30.8M records,
// DESIGN.md §3.10.)
__global__ __launch_bounds__(256) void kPairFlags(const sahara_hit* __restrict__ h, uint64_t n, uint64_t dmin,
                                                  uint64_t dmax, const uint64_t* __restrict__ qoff, uint64_t qidBase,
                                                  uint32_t nq, uint32_t* __restrict__ flag) {
    const HitAt at{h};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const sahara_hit x = h[i];
        uint64_t first = 0, last = n;
        const uint64_t p = pairPartner(x.qid) - qidBase;  // (qidBase is a multiple of 4: no wrap)
        if (p < nq) {
            first = qoff[p];
            last = min(qoff[p + 1], n);
            first = min(first, last);
        }
        flag[i] = pairKeeps(at, x.qid, x.seq_id, x.pos, dmin, dmax, first, last) ? 1u : 0u;
    }
}

// Kept record i goes to dst[num[i] - 1] (dst == nullptr: every record is kept,
// nothing moves, only the count below runs). The pairs that keep a hit: a
// kept record counts iff the kept record before it belongs to another pair
// (qid >> 2). Within a wave that record is the nearest kept lane below, read
// by a shuffle; the first kept lane of a wave finds it as the first record
// whose running count reaches its own less one (a lower bound over num, one
// lane per wave). A wave walks 64 consecutive records, so every lane runs
// every iteration and only loads and stores are predicated.
__global__ __launch_bounds__(256) void kPairGather(const sahara_hit* __restrict__ h, const uint32_t* __restrict__ flag,
                                                   const uint32_t* __restrict__ num, uint64_t n,
                                                   sahara_hit* __restrict__ dst,
                                                   unsigned long long* __restrict__ pairs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t counted = 0;  // (lane 0's: the wave's pairs so far)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool keep = i < n && (dst == nullptr || flag[i] != 0);
        sahara_hit x{};
        uint32_t k = 0;  // the record's index among the kept ones
        if (keep) {
            x = h[i];
            k = dst ? num[i] - 1u : (uint32_t)i;
            if (dst) dst[k] = x;
        }
        const uint64_t keptLanes = __ballot(keep);
        const uint64_t below = keptLanes & ((1ull << lane) - 1ull);
        const uint32_t from = below ? 63u - (uint32_t)__clzll((long long)below) : lane;
        uint64_t prevQid = __shfl(x.qid, (int)from);
        bool first = false;
        if (keep) {
            if (below == 0 && k > 0) {  // the kept record before this wave's first
                uint64_t j = i - 1;
                if (dst) {
                    uint64_t lo = 0, hi = i;  // num is non-decreasing and reaches k at kept record k - 1
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        if (num[mid] < k) lo = mid + 1;
                        else hi = mid;
                    }
                    j = lo;
                }
                prevQid = h[j].qid;
            }
            first = k == 0 || (prevQid >> 2) != (x.qid >> 2);
        }
        counted += (uint32_t)__popcll(__ballot(first));
    }
    // one atomic per wave, after its last record: issued once per 64 records they all meet in
    // one address, and the kernel took 2.59 ms for 30.8M records instead of 0.99 ms
    if (lane == 0 && counted) atomicAdd(pairs, (unsigned long long)counted);
}

}  // namespace

// flag[i] = record i of the batch has a concordant mate in it (kPairFlags): the pair stage's first
// step, and the mate rescue's (rescue.hip), whose anchors are the records without one
void launchPairFlags(const BatchView& v, uint64_t dmin, uint64_t dmax, uint32_t* flag) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((v.rows + 255) / 256, 8192);
    hipLaunchKernelGGL(kPairFlags, dim3(blocks), dim3(256), 0, v.st, v.hits, v.rows, dmin, dmax, v.qoff, v.q0, v.nq,
                       flag);
    SH_HIP(hipGetLastError());
}

// The batch (search.h BatchView: whole hits in canonical order, a pair's four
// qids all in it) reduced in place to the hits with a concordant mate for
// pattern length len and fragments in [minFrag, maxFrag] (maxFrag >= len: the
// call is refused otherwise, capi.cpp). Host-synchronous like lociBatch: the
// kept count sizes the rest of the batch's chain. The number of pairs that
// keep a hit arrives in *hostPairs (pinned) once v.st has passed this call's
// last copy: the caller reads it after the batch's chain.
void pairsBatch(BatchView& v, uint32_t len, uint32_t minFrag, uint32_t maxFrag, PairsBufs& B, uint64_t* hostPairs) {
    *hostPairs = 0;
    const uint64_t rows = v.rows;
    if (rows == 0) return;
    if (rows >= (1ull << 32)) throw Error("more than 2^32 hits in one batch of patterns");  // (the 32-bit running count)
    if (maxFrag < len) throw Error("pairs: max_fragment is below the pattern length (internal)");
    room(B.flag, rows);
    room(B.num, rows);
    B.pairs.reserve(1);
    const PairDist d = pairDist(len, minFrag, maxFrag);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((rows + 255) / 256, 8192);
    launchPairFlags(v, d.dmin, d.dmax, B.flag.ptr);
    const uint64_t kept = scanFlagsCount(B.flag.ptr, B.num.ptr, v);
    if (kept > rows) throw Error("pairs: the kept count is out of range (internal)");
    if (kept == 0) {  // (no rows: no later stage runs on them, nothing reads the segments)
        v.rows = 0;
        return;
    }
    SH_HIP(hipMemsetAsync(B.pairs.ptr, 0, sizeof(unsigned long long), v.st));
    const bool all = kept == rows;  // nothing to drop: the records and the segments stand, the pairs are counted
    if (!all) room(v.scratch, kept);
    hipLaunchKernelGGL(kPairGather, dim3(blocks), dim3(256), 0, v.st, v.hits, B.flag.ptr, B.num.ptr, rows,
                       all ? nullptr : v.scratch.ptr, B.pairs.ptr);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(hostPairs, B.pairs.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, v.st));
    if (!all) replaceBatch(v, kept);
}

}  // namespace sahara
