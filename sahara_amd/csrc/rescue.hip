// rescue.hip — the mate rescue of a batch's chain (docs/semantics.md "Mate
// rescue"): between the loci stage and the pair stage, a hit
// whose partner query has no hit in its fragment window (an anchor) gets that
// window scanned for the partner's pattern with a larger error bound, and
// what the scans find joins the batch's hits in canonical order (gfx950).
//
//   kPairFlags          (pairs.hip) record i has a mate?            -> flag[i]
//   kRescueAnchorFlags  no mate, first of its position, a window    -> flag[i]
//   rocPRIM scan, kRescueCap   (cap A > 0) a query with more than A anchors loses them
//   rocPRIM select      the anchors' indices                        -> anchors[0 .. na)
//   kRescueScan         one wave per anchor: the least (errors, start) of its window
//                                                                   -> found[a], or a sentinel
//   rocPRIM merge_sort, unique, merge   the distinct records, merged with the batch's
//
// The scan is align_core.h's table build alone (no traceback), one start per
// lane and 64 starts per round, against the resident text and the batch's
// staged patterns; the pieces of the rule are rescue_core.h's.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "align_device.h"
#include "rescue_core.h"
#include "search_device.h"

namespace sahara {
namespace {

constexpr uint32_t kRescueWave = kAlignLanes;  // one wave per anchor (align_device.h: its table in LDS)
enum RescueWord : uint32_t { kRwAnchors = 0, kRwCapped, kRwStarts, kRwDistinct, kRwRescued, kRescueWords };

static_assert(kRescueMaxWindow == SAHARA_RESCUE_MAX_WINDOW && kRescueMaxWindow <= 0x10000u,
              "rescue_core.h mirrors the ABI; a start's index is 16 bits of the result word");

// symbols of record `seq` (its '$' not counted); 0 for a record the part does not have
__device__ __forceinline__ uint64_t recLenOf(const uint64_t* __restrict__ recStarts, uint32_t nrec, uint64_t textLen,
                                             uint32_t seq) {
    if (seq >= nrec) return 0;
    const uint64_t end = seq + 1 < nrec ? recStarts[seq + 1] : textLen;
    return end - recStarts[seq] - 1;
}

// flag[i]: in, record i has a mate (kPairFlags); out, it is an anchor
__global__ __launch_bounds__(256) void kRescueAnchorFlags(const sahara_hit* __restrict__ h, uint64_t n, uint64_t dmin,
                                                          uint64_t dmax, const uint64_t* __restrict__ recStarts,
                                                          uint32_t nrec, uint64_t textLen, uint32_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const sahara_hit x = h[i];
        const sahara_hit p = i ? h[i - 1] : x;
        flag[i] = rescueIsAnchor(i == 0, p.qid, p.seq_id, p.pos, x.qid, x.seq_id, x.pos, flag[i] != 0, dmin, dmax,
                                 recLenOf(recStarts, nrec, textLen, x.seq_id))
                      ? 1u : 0u;
    }
}

// The cap: num is the anchor flags' inclusive sum, so a query's anchors are
// the difference over its segment [qoff[q], qoff[q + 1]). A query with more
// than `most` loses its flags; its first anchor counts it.
__global__ __launch_bounds__(256) void kRescueCap(const sahara_hit* __restrict__ h, uint64_t n,
                                                  const uint32_t* __restrict__ num, const uint64_t* __restrict__ qoff,
                                                  uint64_t qidBase, uint32_t nq, uint32_t most,
                                                  uint32_t* __restrict__ flag, unsigned long long* __restrict__ capped) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[i]) continue;
        const uint64_t q = h[i].qid - qidBase;
        if (q >= nq) continue;
        const uint64_t a = min(qoff[q], n), b = min(qoff[q + 1], n);
        const uint32_t before = a ? num[a - 1] : 0u;
        const uint32_t mine = (b ? num[b - 1] : 0u) - before;
        if (mine <= most) continue;
        flag[i] = 0;
        if (num[i] - before == 1u) atomicAdd(capped, 1ull);
    }
}

struct ScanArgs {
    const sahara_hit* h;
    const uint32_t* anchors;
    const uint64_t* recStarts;
    uint32_t nrec;
    uint64_t textLen;
    const uint4* text3;
    uint32_t text3Bytes;
    const uint4* pats3;
    uint32_t patBlocks;
    uint64_t qidBase;
    uint32_t nq;
    uint32_t m, maxErr, edit;
    uint64_t dmin, dmax;
    sahara_hit* found;
    unsigned long long* starts;
};

// One wave per anchor. Lane l takes the window's starts l, l + 64, ...; after
// each round of 64 the wave reduces the lanes' (errors, start) words to their
// least. Ties go to the smaller start and later rounds hold larger starts
// only, so a later round needs fewer errors to win: it runs with the bound
// one below the best so far, and no round runs once that is 0.
__global__ __launch_bounds__(kRescueWave) void kRescueScan(ScanArgs a) {
    extern __shared__ int16_t rescueLds[];
    const uint32_t lane = threadIdx.x;
    const sahara_hit x = a.h[a.anchors[blockIdx.x]];
    const uint64_t recLen = recLenOf(a.recStarts, a.nrec, a.textLen, x.seq_id);
    const RescueWindow w = rescueWindow(x.qid, x.pos, a.dmin, a.dmax, recLen);
    const uint64_t partner = pairPartner(x.qid) - a.qidBase;
    uint32_t best = kRescueNone;
    if (w.any && partner < a.nq) {  // (both hold for an anchor of a batch of whole pairs)
        const uint32_t count = (uint32_t)min(w.hi - w.lo + 1, (uint64_t)kRescueMaxWindow);
        const uint32_t p = __builtin_amdgcn_readfirstlane((uint32_t)partner);
        // the partner's blocks and the one after them (read and masked, align_core.h), within the batch's
        const uint32_t patBytes = (uint32_t)min((uint64_t)(a.nq - p) * a.patBlocks, (uint64_t)a.patBlocks + 1) * 16u;
        BufBlocks text{alignBufferOf(a.text3, a.text3Bytes)};
        BufBlocks pat{alignBufferOf(a.pats3 + (uint64_t)p * a.patBlocks, patBytes)};
        LaneTable L{rescueLds + lane};
        const uint32_t g0 = (uint32_t)(a.recStarts[x.seq_id] + w.lo);
        int bound = (int)a.maxErr;
        for (uint32_t base = 0; base < count && bound >= 0; base += kRescueWave) {
            const uint32_t at = base + lane;
            uint32_t key = kRescueNone;
            if (at < count) {
                const int e = alignTable(pat, text, g0 + at, a.m, (uint32_t)bound, a.edit != 0, L);
                if (e >= 0) key = rescueKey((uint32_t)e, at);
            }
            for (int off = 32; off; off >>= 1) key = rescueBest(key, (uint32_t)__shfl_xor((int)key, off));
            if (key != kRescueNone) {
                best = rescueBest(best, key);
                bound = (int)rescueKeyErr(best) - 1;
            }
        }
        if (lane == 0) atomicAdd(a.starts, (unsigned long long)count);
    }
    if (lane == 0) {
        sahara_hit r{~0ull, ~0u, ~0u, ~0ull};  // the sentinel: above every record
        if (best != kRescueNone) r = sahara_hit{pairPartner(x.qid), x.seq_id, rescueKeyErr(best), w.lo + rescueKeyAt(best)};
        a.found[blockIdx.x] = r;
    }
}

struct HitSame {  // (two anchors that find one position find one e*)
    __host__ __device__ bool operator()(const sahara_hit& a, const sahara_hit& b) const {
        return a.qid == b.qid && a.seq_id == b.seq_id && a.pos == b.pos;
    }
};

// the distinct records less the sentinel, which sorts last
__global__ void kRescueCount(const sahara_hit* __restrict__ sorted, unsigned long long* __restrict__ words) {
    const unsigned long long n = words[kRwDistinct];
    words[kRwRescued] = n && sorted[n - 1].qid == ~0ull ? n - 1 : n;
}

}  // namespace

// The stage's first half: the anchors of the batch (search.h BatchView: whole
// hits in canonical order) found and scanned, the distinct rescued records
// left in B.found in canonical order and their number returned; the stage's
// counts join `total`. Host-synchronous like pairsBatch: the number sizes
// what the caller grows before the merge.
uint64_t rescueFind(const BatchView& v, const RescueIn& in, RescueBufs& B, sahara_rescue_stats& total) {
    const sahara_hit* const h = v.hits;
    const uint64_t rows = v.rows;
    const hipStream_t st = v.st;
    if (rows == 0) return 0;
    if (rows >= (1ull << 32)) throw Error("more than 2^32 hits in one batch of patterns");  // (32-bit indices and sums)
    if (in.maxFrag < in.len || in.maxErr == 0 || in.maxErr > kAlignMaxErr || in.len > kAlignMaxLen)
        throw Error("rescue: a setting out of range reached the stage (internal)");
    const PairDist d = pairDist(in.len, in.minFrag, in.maxFrag);
    if (d.dmax - d.dmin >= kRescueMaxWindow) throw Error("rescue: the fragment window is too wide (internal)");
    room(B.flag, rows);
    room(B.anchors, rows);
    B.words.reserve(kRescueWords);
    B.host.reserve(kRescueWords);
    SH_HIP(hipMemsetAsync(B.words.ptr, 0, kRescueWords * sizeof(unsigned long long), st));
    launchPairFlags(v, d.dmin, d.dmax, B.flag.ptr);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((rows + 255) / 256, 8192);
    hipLaunchKernelGGL(kRescueAnchorFlags, dim3(blocks), dim3(256), 0, st, h, rows, d.dmin, d.dmax, in.recStarts, in.nrec,
                       in.textLen, B.flag.ptr);
    SH_HIP(hipGetLastError());
    if (in.maxAnchors) {
        room(B.num, rows);
        withTemp(v.tmp, [&](void* temp, size_t& bytes) {
            return rocprim::inclusive_scan(temp, bytes, B.flag.ptr, B.num.ptr, (size_t)rows, rocprim::plus<uint32_t>(), st);
        });
        hipLaunchKernelGGL(kRescueCap, dim3(blocks), dim3(256), 0, st, h, rows, B.num.ptr, v.qoff, v.q0, v.nq,
                           in.maxAnchors, B.flag.ptr, B.words.ptr + kRwCapped);
        SH_HIP(hipGetLastError());
    }
    const rocprim::counting_iterator<uint32_t> index(0u);
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::select(temp, bytes, index, B.flag.ptr, B.anchors.ptr, B.words.ptr + kRwAnchors, (size_t)rows, st);
    });
    SH_HIP(hipMemcpyAsync(B.host.ptr, B.words.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    const uint64_t na = B.host.ptr[kRwAnchors];
    total.capped_queries += B.host.ptr[kRwCapped];
    if (na > rows) throw Error("rescue: the anchor count is out of range (internal)");
    total.anchors += na;
    if (na == 0) return 0;
    if (na > 0x7FFFFFFFull) throw Error("rescue: too many anchors in one batch of patterns");
    room(B.found, na);
    room(B.sorted, na);
    ScanArgs a{};
    a.h = h;
    a.anchors = B.anchors.ptr;
    a.recStarts = in.recStarts;
    a.nrec = in.nrec;
    a.textLen = in.textLen;
    a.text3 = in.text3;
    a.text3Bytes = (uint32_t)std::min<uint64_t>(text3Blocks(in.textLen) * 16, 0xFFFFFF00ull);
    a.pats3 = in.pats3;
    a.patBlocks = in.patBlocks;
    a.qidBase = v.q0;
    a.nq = v.nq;
    a.m = in.len;
    a.maxErr = in.maxErr;
    a.edit = in.edit ? 1u : 0u;
    a.dmin = d.dmin;
    a.dmax = d.dmax;
    a.found = B.found.ptr;
    a.starts = B.words.ptr + kRwStarts;
    const size_t lds = alignTableBytes(in.maxErr, in.edit);
    hipLaunchKernelGGL(kRescueScan, dim3((unsigned)na), dim3(kRescueWave), lds, st, a);
    SH_HIP(hipGetLastError());
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::merge_sort(temp, bytes, B.found.ptr, B.sorted.ptr, (size_t)na, HitLess(), st);
    });
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::unique(temp, bytes, B.sorted.ptr, B.found.ptr, B.words.ptr + kRwDistinct, (size_t)na, HitSame(), st);
    });
    hipLaunchKernelGGL(kRescueCount, dim3(1), dim3(1), 0, st, B.found.ptr, B.words.ptr);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(B.host.ptr, B.words.ptr, kRescueWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    total.starts += B.host.ptr[kRwStarts];
    const uint64_t r = B.host.ptr[kRwRescued];
    if (r > na) throw Error("rescue: the rescued count is out of range (internal)");
    total.rescued += r;
    return r;
}

// The second half: the r records rescueFind left in B.found merged into the
// batch's (v.hits has room for v.rows + r records). H and R share no position
// (a record at a rescued one would have been the anchor's mate): a plain
// merge keeps the canonical order.
void rescueMerge(BatchView& v, uint64_t r, RescueBufs& B) {
    if (r == 0) return;
    const uint64_t rows = v.rows;
    room(v.scratch, rows + r);
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::merge(temp, bytes, v.hits, B.found.ptr, v.scratch.ptr, (size_t)rows, (size_t)r, HitLess(), v.st);
    });
    replaceBatch(v, rows + r);
}

}  // namespace sahara
