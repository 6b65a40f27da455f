// loci.hip — the loci stage of a batch's chain (docs/semantics.md "Loci",
// DESIGN.md §3.9): a batch's whole hits, in canonical order after the sort,
// cut down to one record per locus before anything leaves the device
// (gfx950). Work is per hit: a query inside a repeat has 10^4..10^5 rows, and
// a lane per query would serialise the batch on it.
//
//   kLociHeads    record i starts a locus?           -> flag[i]
//   rocPRIM scan  inclusive sum of the flags         -> num[i] = locus of i, + 1; num[rows - 1] = loci
//                 (hits.hip scanFlagsCount)
//   kLociReduce   min over each locus of (err, i)    -> best[locus]
//   kLociGather   the representatives, in order      -> scratch, copied back over the batch
//                 (hits.hip replaceBatch)
//
// The predicate and the key are loci_core.h's.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "loci_core.h"
#include "search_device.h"

namespace sahara {
namespace {

// Both per-hit kernels walk the records a wave at a time: `base` is the wave's
// first record, the same for its 64 lanes, so every lane runs every iteration
// (the shuffles and the ballot need all of them) and only the loads, stores
// and atomics are predicated on i < n.
__device__ __forceinline__ uint64_t waveBase(uint32_t lane) {
    return (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);
}

// The neighbour's fields come from the lane below; lane 0 reads record i - 1
// itself (the last record of the wave before, or of another workgroup).
__global__ __launch_bounds__(256) void kLociHeads(const sahara_hit* __restrict__ h, uint64_t n, uint32_t window,
                                                  uint32_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = waveBase(lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        sahara_hit x{};
        if (valid) x = h[i];
        uint64_t pq = __shfl_up(x.qid, 1);
        uint32_t ps = __shfl_up(x.seq_id, 1);
        uint64_t pp = __shfl_up(x.pos, 1);
        if (lane == 0 && valid && i > 0) {
            const sahara_hit p = h[i - 1];
            pq = p.qid;
            ps = p.seq_id;
            pp = p.pos;
        }
        if (valid) flag[i] = i == 0 || lociHead(pq, ps, pp, x.qid, x.seq_id, x.pos, window) ? 1u : 0u;
    }
}

// Locus numbers do not decrease from lane to lane, so the lanes of one locus
// are a run: a segmented min-scan over the wave (six shuffle steps; a lane
// takes the value `off` lanes below only if that lane is in its run, which
// the ballot of the runs' first lanes tells) leaves each run's minimum in its
// last lane, and only that lane issues the atomic. A locus that spans waves
// or workgroups meets in best[locus] (all ones on entry).
__global__ __launch_bounds__(256) void kLociReduce(const sahara_hit* __restrict__ h, const uint32_t* __restrict__ num,
                                                   uint64_t n, unsigned long long* __restrict__ best) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = waveBase(lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        // (lanes past the last record: a run of their own behind it, which issues nothing)
        const uint32_t locus = valid ? num[i] - 1u : 0xFFFFFFFFu;
        uint64_t key = valid ? lociKey(h[i].err, (uint32_t)i) : kLociNoKey;
        const uint32_t below = __shfl_up(locus, 1);
        const uint64_t firsts = __ballot(lane == 0 || below != locus);
        const uint32_t first = 63u - (uint32_t)__clzll((long long)(firsts & (~0ull >> (63u - lane))));
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint64_t o = __shfl_up(key, off);
            if (lane >= first + off) key = o < key ? o : key;
        }
        const bool last = lane == 63u || ((firsts >> (lane + 1u)) & 1ull);
        if (valid && last) atomicMin(best + locus, (unsigned long long)key);
    }
}

__global__ void kLociGather(const sahara_hit* __restrict__ h, const unsigned long long* __restrict__ best,
                            uint64_t loci, sahara_hit* __restrict__ dst) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < loci; l += (uint64_t)gridDim.x * blockDim.x)
        dst[l] = h[lociKeyIndex(best[l])];
}

}  // namespace

// The batch (search.h BatchView: whole hits in canonical order) reduced in
// place to one record per locus for `window`. Host-synchronous: the locus
// count sizes the rest of the batch's chain.
void lociBatch(BatchView& v, uint32_t window, LociBufs& B) {
    const uint64_t rows = v.rows;
    if (rows == 0) return;
    if (rows >= (1ull << 32)) throw Error("more than 2^32 hits in one batch of patterns");  // (the key's index)
    room(B.flag, rows);
    room(B.num, rows);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((rows + 255) / 256, 8192);
    hipLaunchKernelGGL(kLociHeads, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, window, B.flag.ptr);
    SH_HIP(hipGetLastError());
    const uint64_t loci = scanFlagsCount(B.flag.ptr, B.num.ptr, v);
    if (loci == 0 || loci > rows) throw Error("loci: the locus count is out of range (internal)");
    if (loci == rows) return;  // every record is a locus of its own: nothing to drop, the segments stand
    room(B.best, loci);
    room(v.scratch, loci);
    SH_HIP(hipMemsetAsync(B.best.ptr, 0xFF, loci * sizeof(unsigned long long), v.st));
    hipLaunchKernelGGL(kLociReduce, dim3(blocks), dim3(256), 0, v.st, v.hits, B.num.ptr, rows, B.best.ptr);
    SH_HIP(hipGetLastError());
    const uint32_t gblocks = (uint32_t)std::min<uint64_t>((loci + 255) / 256, 8192);
    hipLaunchKernelGGL(kLociGather, dim3(gblocks), dim3(256), 0, v.st, v.hits, B.best.ptr, loci, v.scratch.ptr);
    SH_HIP(hipGetLastError());
    replaceBatch(v, loci);
}

}  // namespace sahara
