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
// In best mode (docs/semantics.md "Best pairs") four more kernels cut the
// flags down to each pair's least-error placements before the scan and write
// a summary per pair after it: see "best mode" below. With links on
// (docs/semantics.md "Pair links") two more write a link per kept record
// before the gather: see "links" below.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "best_pairs_core.h"
#include "pair_links_core.h"
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

// ---- best mode (docs/semantics.md "Best pairs"): between
// kPairFlags and the scan, the flags are cut down to each pair's least-error
// placements, and after the scan one lane per pair writes the pair's summary.
//
//   kBestBlocks   err of record i as a byte; its least over each aligned block of 64  -> err8[i], blk[i / 64]
//   kBestScore    record i with a mate: its mates' index range (two lower bounds), the
//                 least err in it (bestRangeMin), m[i] = the sum; atomicMin into best[pair]
//   kBestFlags    flag[i] = first of its position && m[i] <= best[pair] + delta;
//                 atomicMin of the other first-of-position scores into next[pair]
//   kBestSummary  (after the scan) per pair: best, next, the kept records of its even
//                 and odd qids from num at its segments' ends                          -> sum[pair]
//
// The per-record kernels walk the records a wave at a time, as loci.hip's do:
// every lane runs every iteration, only loads, stores and atomics are predicated.

struct ErrAt {
    const uint8_t* e;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return e[i]; }
};

// The minimum of `key` over each run of lanes with equal `run` (runs do not
// decrease from lane to lane: the records are sorted by qid), left in the
// run's last lane: the segmented min-scan of kLociReduce. A tandem run puts
// thousands of records on one pair: one atomic per run and wave, not per record.
struct RunMin {
    uint32_t key;
    bool last;
};
__device__ __forceinline__ RunMin runMin(uint32_t key, uint32_t run, uint32_t lane) {
    const uint32_t below = __shfl_up(run, 1);
    const uint64_t firsts = __ballot(lane == 0 || below != run);
    const uint32_t first = 63u - (uint32_t)__clzll((long long)(firsts & (~0ull >> (63u - lane))));
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(key, off);
        if (lane >= first + off) key = o < key ? o : key;
    }
    return {key, lane == 63u || ((firsts >> (lane + 1u)) & 1ull) != 0};
}

__global__ __launch_bounds__(256) void kBestBlocks(const sahara_hit* __restrict__ h, uint64_t n,
                                                   uint8_t* __restrict__ err8, uint8_t* __restrict__ blk) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        uint32_t e = kBestNone;
        if (i < n) {
            e = min(h[i].err, kBestNone - 1u);
            err8[i] = (uint8_t)e;
        }
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1) e = min(e, (uint32_t)__shfl_xor(e, (int)off));
        if (lane == 0) blk[base / kBestBlock] = (uint8_t)e;  // (base is a multiple of 64)
    }
}

__global__ __launch_bounds__(256) void kBestScore(const sahara_hit* __restrict__ h, uint64_t n, uint64_t dmin,
                                                  uint64_t dmax, const uint64_t* __restrict__ qoff, uint64_t qidBase,
                                                  uint32_t nq, const uint32_t* __restrict__ flag,
                                                  const uint8_t* __restrict__ err8, const uint8_t* __restrict__ blk,
                                                  uint8_t* __restrict__ m, uint32_t* __restrict__ best) {
    const HitAt at{h};
    const ErrAt errAt{err8}, blockAt{blk};
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        uint32_t score = kBestNone, pair = 0xFFFFFFFFu;
        if (valid) {
            const sahara_hit x = h[i];
            const uint64_t q = x.qid - qidBase;
            if (q < nq) pair = (uint32_t)(q >> 2);
            const uint64_t p = pairPartner(x.qid) - qidBase;
            if (flag[i] != 0 && p < nq) {  // (a mate lies in the partner's segment: kPairFlags found it there)
                const uint64_t last = min(qoff[p + 1], n), first = min(qoff[p], last);
                const BestRange r = bestMateRange(at, x.qid, x.seq_id, x.pos, dmin, dmax, first, last);
                score = bestScore(min(x.err, kBestNone - 1u), bestRangeMin(errAt, blockAt, r.lb, r.ub));
            }
            m[i] = (uint8_t)min(score, kBestNone);
        }
        const RunMin r = runMin(score, pair, lane);
        if (r.last && r.key < kBestNone && pair != 0xFFFFFFFFu) atomicMin(best + pair, r.key);
    }
}

// The neighbour's fields come from the lane below; lane 0 reads record i - 1 itself (kLociHeads).
__global__ __launch_bounds__(256) void kBestFlags(const sahara_hit* __restrict__ h, uint64_t n, uint64_t qidBase,
                                                  uint32_t nq, uint32_t delta, const uint8_t* __restrict__ m,
                                                  const uint32_t* __restrict__ best, uint32_t* __restrict__ next,
                                                  uint32_t* __restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
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
        uint32_t pair = 0xFFFFFFFFu, other = kBestNone;
        if (valid) {
            const bool firstOfPos = i == 0 || pq != x.qid || ps != x.seq_id || pp != x.pos;
            const uint64_t q = x.qid - qidBase;
            const uint32_t score = m[i];
            bool keep = false;
            if (q < nq && score != kBestNone) {  // (then best[pair] has a value: at most this score)
                pair = (uint32_t)(q >> 2);
                const uint32_t b = best[pair];
                keep = bestKeeps(firstOfPos, score, b, delta);
                if (firstOfPos && score > b) other = score;
            } else if (q < nq) {
                pair = (uint32_t)(q >> 2);
            }
            flag[i] = keep ? 1u : 0u;
        }
        const RunMin r = runMin(other, pair, lane);
        if (r.last && r.key < kBestNone && pair != 0xFFFFFFFFu) atomicMin(next + pair, r.key);
    }
}

// One lane per pair, no atomics: the kept records of query q are num's growth
// over its segment [qoff[q], qoff[q + 1]), the flags' inclusive sum at the
// segment's ends (the segments of the records the flags were made for). The
// grid holds every pair (a batch has fewer than 2^30: the launch has no cap
// and the kernel no loop).
__global__ __launch_bounds__(256) void kBestSummary(const uint32_t* __restrict__ num, uint64_t n,
                                                    const uint64_t* __restrict__ qoff, uint32_t npairs,
                                                    const uint32_t* __restrict__ best,
                                                    const uint32_t* __restrict__ next,
                                                    sahara_pair_summary* __restrict__ sum) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    uint32_t cnt[2] = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t e = min(qoff[4 * (uint64_t)p + k + 1], n), b = min(qoff[4 * (uint64_t)p + k], e);
        cnt[k & 1u] += (e ? num[e - 1] : 0u) - (b ? num[b - 1] : 0u);
    }
    sahara_pair_summary s;
    s.best = (uint8_t)min(best[p], kBestNone);
    s.next = (uint8_t)min(next[p], kBestNone);
    s.n_fwd = (uint16_t)min(cnt[0], 65535u);
    s.n_rev = (uint16_t)min(cnt[1], 65535u);
    s.reserved = 0;
    sum[p] = s;
}

// ---- links (docs/semantics.md "Pair links"): after the scan
// and the summary, before the gather, every kept record gets a link.
//
//   kLinkMates  kept record i: its mate range again and the first record in it with the
//               least err (bestRangeArgMin)                                  -> mate[i];
//               atomicMin of (m, i) over the kept even-qid records           -> key[pair];
//               the kept records with m == s1, even and odd qids apart       -> ties[2 pair], ties[2 pair + 1]
//   kLinkWrite  kept record i -> link[num[i] - 1]: the mate's offset among the kept records,
//               m, primary (i is the key's record, or that record's mate), the pair's MAPQ
//
// The atomics are per run and wave, as kBestScore's: a tandem run puts hundreds
// of kept records on one pair.

// The lanes at which a run of equal `run` starts and ends, for the segmented scans below (runMin's)
struct RunEnds {
    uint32_t first;  // the first lane of this lane's run
    bool last;       // this lane is its run's last
};
__device__ __forceinline__ RunEnds runEnds(uint32_t run, uint32_t lane) {
    const uint32_t below = __shfl_up(run, 1);
    const uint64_t firsts = __ballot(lane == 0 || below != run);
    const uint32_t first = 63u - (uint32_t)__clzll((long long)(firsts & (~0ull >> (63u - lane))));
    return {first, lane == 63u || ((firsts >> (lane + 1u)) & 1ull) != 0};
}

__global__ __launch_bounds__(256) void kLinkMates(const sahara_hit* __restrict__ h, uint64_t n, uint64_t dmin,
                                                  uint64_t dmax, const uint64_t* __restrict__ qoff, uint64_t qidBase,
                                                  uint32_t nq, const uint32_t* __restrict__ flag,
                                                  const uint8_t* __restrict__ err8, const uint8_t* __restrict__ blk,
                                                  const uint8_t* __restrict__ m, const uint32_t* __restrict__ best,
                                                  uint32_t* __restrict__ mate, unsigned long long* __restrict__ key,
                                                  uint32_t* __restrict__ ties) {
    const HitAt at{h};
    const ErrAt errAt{err8}, blockAt{blk};
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        uint32_t pair = 0xFFFFFFFFu, tie = 0;  // tie: 1 for an even qid with m == s1, 1 << 16 for an odd one
        unsigned long long k = kLinkNoKey;
        if (i < n && flag[i] != 0) {  // kept: it has a score, so its partner's segment lies in the batch
            const sahara_hit x = h[i];
            const uint64_t q = x.qid - qidBase, p = pairPartner(x.qid) - qidBase;
            if (q < nq && p < nq) {
                pair = (uint32_t)(q >> 2);
                const uint64_t last = min(qoff[p + 1], n), first = min(qoff[p], last);
                const BestRange r = bestMateRange(at, x.qid, x.seq_id, x.pos, dmin, dmax, first, last);
                const uint32_t score = m[i];
                const uint64_t j = bestRangeArgMin(errAt, blockAt, r.lb, r.ub, score - min(x.err, kBestNone - 1u));
                mate[i] = j < r.ub ? (uint32_t)j : (uint32_t)i;  // (always j < ub: m[i] was made from this range's least)
                const bool odd = (x.qid & 1ull) != 0;
                if (!odd) k = pairPrimaryKey(score, (uint32_t)i);
                if (score == best[pair]) tie = odd ? 1u << 16 : 1u;
            }
        }
        const RunEnds r = runEnds(pair, lane);
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const unsigned long long ok = __shfl_up(k, off);
            const uint32_t ot = __shfl_up(tie, off);
            if (lane >= r.first + off) {
                k = ok < k ? ok : k;
                tie += ot;  // (at most 64 in either half)
            }
        }
        if (r.last && pair != 0xFFFFFFFFu) {
            if (k != kLinkNoKey) atomicMin(key + pair, k);
            if (tie & 0xFFFFu) atomicAdd(ties + 2 * (uint64_t)pair, tie & 0xFFFFu);
            if (tie >> 16) atomicAdd(ties + 2 * (uint64_t)pair + 1, tie >> 16);
        }
    }
}

__global__ __launch_bounds__(256) void kLinkWrite(const sahara_hit* __restrict__ h, uint64_t n, uint64_t qidBase,
                                                  uint32_t nq, const uint32_t* __restrict__ flag,
                                                  const uint32_t* __restrict__ num, const uint32_t* __restrict__ mate,
                                                  const uint8_t* __restrict__ m, const uint32_t* __restrict__ best,
                                                  const uint32_t* __restrict__ next,
                                                  const unsigned long long* __restrict__ key,
                                                  const uint32_t* __restrict__ ties, uint64_t kept,
                                                  sahara_pair_link* __restrict__ link) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const uint64_t i = base + lane;
        if (i >= n || flag[i] == 0) continue;  // (no wave-wide step below: a lane may sit an iteration out)
        const uint64_t qid = h[i].qid, q = qid - qidBase;
        const uint32_t self = num[i] - 1u;
        if (q >= nq || self >= kept) continue;
        const uint32_t pair = (uint32_t)(q >> 2), j = mate[i];  // (j < n: kLinkMates wrote a row of the batch)
        const unsigned long long k = key[pair];
        bool primary = false;
        if (k != kLinkNoKey) {
            const uint32_t ki = pairPrimaryIndex(k);  // (a row of the batch as well, and kept: mate[ki] is written)
            primary = (qid & 1ull) == 0 ? ki == (uint32_t)i : mate[ki] == (uint32_t)i;
        }
        sahara_pair_link x;
        x.mate = (int32_t)((num[j] - 1u) - self);
        x.score = m[i];
        x.mapq = primary ? (uint8_t)pairMapq(best[pair], next[pair], max(ties[2 * (uint64_t)pair], ties[2 * (uint64_t)pair + 1])) : 0;
        x.flags = primary ? kLinkPrimary : 0;
        x.reserved = 0;
        link[self] = x;
    }
}

// The pinned links grown to hold `need`, the first `keep` kept: the copies of the earlier batches, all on
// st, are waited for first. Grown by half again, so that a call of many batches allocates a few times.
void growLinks(PinnedBuf<sahara_pair_link>& buf, uint64_t need, uint64_t keep, hipStream_t st) {
    if (need <= buf.cap) return;
    SH_HIP(hipStreamSynchronize(st));
    PinnedBuf<sahara_pair_link> grown;
    grown.reserve(std::max<uint64_t>(need + need / 2, 1024));
    if (keep) std::copy_n(buf.ptr, keep, grown.ptr);
    buf = std::move(grown);
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
// last copy: the caller reads it after the batch's chain. best != nullptr:
// best mode, which keeps of those hits each pair's least-error placements
// (within best->delta) and copies the batch's pair summaries to
// best->summary[q0 / 4 ..] (pinned, read after the batch's chain as well);
// best->links != nullptr: and the kept records' links to the call's links
// from best->links->at on (pinned too, grown here once the count is known).
void pairsBatch(BatchView& v, uint32_t len, uint32_t minFrag, uint32_t maxFrag, PairsBufs& B, uint64_t* hostPairs,
                const BestPairsIn* best) {
    *hostPairs = 0;
    const uint64_t rows = v.rows;
    if (rows == 0) return;
    if (rows >= (1ull << 32)) throw Error("more than 2^32 hits in one batch of patterns");  // (the 32-bit running count)
    if (maxFrag < len) throw Error("pairs: max_fragment is below the pattern length (internal)");
    if (best && (v.nq % 4 || v.q0 % 4)) throw Error("best pairs: a batch is not cut at whole pairs (internal)");
    room(B.flag, rows);
    room(B.num, rows);
    B.pairs.reserve(1);
    const PairDist d = pairDist(len, minFrag, maxFrag);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((rows + 255) / 256, 8192);
    launchPairFlags(v, d.dmin, d.dmax, B.flag.ptr);
    const uint32_t npairs = v.nq / 4;
    if (best) {  // the flags cut down to the least-error placements; best[] and next[] start as "no value"
        room(B.err8, rows);
        room(B.score, rows);
        room(B.blk, (rows + kBestBlock - 1) / kBestBlock);
        room(B.best, 2 * (uint64_t)npairs);
        room(B.sum, npairs);
        uint32_t* const next = B.best.ptr + npairs;
        SH_HIP(hipMemsetAsync(B.best.ptr, 0xFF, 2 * (size_t)npairs * sizeof(uint32_t), v.st));
        hipLaunchKernelGGL(kBestBlocks, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, B.err8.ptr, B.blk.ptr);
        SH_HIP(hipGetLastError());
        hipLaunchKernelGGL(kBestScore, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, d.dmin, d.dmax, v.qoff, v.q0, v.nq,
                           B.flag.ptr, B.err8.ptr, B.blk.ptr, B.score.ptr, B.best.ptr);
        SH_HIP(hipGetLastError());
        hipLaunchKernelGGL(kBestFlags, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, v.q0, v.nq, best->delta,
                           B.score.ptr, B.best.ptr, next, B.flag.ptr);
        SH_HIP(hipGetLastError());
    }
    const uint64_t kept = scanFlagsCount(B.flag.ptr, B.num.ptr, v);
    if (kept > rows) throw Error("pairs: the kept count is out of range (internal)");
    if (best) {  // before replaceBatch writes the segments again: the counts are taken at the old ones
        hipLaunchKernelGGL(kBestSummary, dim3((npairs + 255) / 256), dim3(256), 0, v.st, B.num.ptr, rows, v.qoff, npairs, B.best.ptr,
                           B.best.ptr + npairs, B.sum.ptr);
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(best->summary + v.q0 / 4, B.sum.ptr, (size_t)npairs * sizeof(sahara_pair_summary),
                              hipMemcpyDeviceToHost, v.st));
    }
    B.linkTimed = false;
    if (best && best->links && kept) {  // the kept records' links, while the flags, the scores and the old rows stand
        room(B.mate, rows);
        room(B.key, npairs);
        room(B.ties, 2 * (uint64_t)npairs);
        room(B.link, kept);
        if (!B.linkStart.e) {
            B.linkStart = Event(hipEventDefault);
            B.linkDone = Event(hipEventDefault);
        }
        SH_HIP(hipMemsetAsync(B.key.ptr, 0xFF, (size_t)npairs * sizeof(unsigned long long), v.st));
        SH_HIP(hipMemsetAsync(B.ties.ptr, 0, 2 * (size_t)npairs * sizeof(uint32_t), v.st));
        SH_HIP(hipEventRecord(B.linkStart, v.st));
        hipLaunchKernelGGL(kLinkMates, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, d.dmin, d.dmax, v.qoff, v.q0, v.nq,
                           B.flag.ptr, B.err8.ptr, B.blk.ptr, B.score.ptr, B.best.ptr, B.mate.ptr, B.key.ptr, B.ties.ptr);
        SH_HIP(hipGetLastError());
        hipLaunchKernelGGL(kLinkWrite, dim3(blocks), dim3(256), 0, v.st, v.hits, rows, v.q0, v.nq, B.flag.ptr, B.num.ptr,
                           B.mate.ptr, B.score.ptr, B.best.ptr, B.best.ptr + npairs, B.key.ptr, B.ties.ptr, kept,
                           B.link.ptr);
        SH_HIP(hipGetLastError());
        SH_HIP(hipEventRecord(B.linkDone, v.st));
        B.linkTimed = true;
        growLinks(*best->links->buf, best->links->at + kept, best->links->at, v.st);
        SH_HIP(hipMemcpyAsync(best->links->buf->ptr + best->links->at, B.link.ptr, (size_t)kept * sizeof(sahara_pair_link),
                              hipMemcpyDeviceToHost, v.st));
    }
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
