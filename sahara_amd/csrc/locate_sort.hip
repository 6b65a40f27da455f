// locate_sort.hip — the locate chain of a batch (gfx950): per-query segments
// from the row counts, kLocate, the tiered sort into canonical order.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "search_device.h"

namespace sahara {
namespace {

__device__ __forceinline__ uint32_t pick5(const uint32_t v[5], uint32_t i) {
    uint32_t r = v[0];
    r = i == 1 ? v[1] : r;
    r = i == 2 ? v[2] : r;
    r = i == 3 ? v[3] : r;
    r = i == 4 ? v[4] : r;
    return r;
}

// ================================================================ locate ====

// Segment tiers: <= kSmallSeg rows sorted in a lane's registers,
// <= kMediumSeg by a wave (one key per lane, bitonic over shuffles), longer
// ones by the segmented radix sort.
constexpr uint32_t kSmallSeg = 8;
constexpr uint32_t kMediumSeg = 64;
// long segments of <= kLdsSeg rows: one workgroup each, bitonic sort in 16 KB
// of LDS (kSortBigLds); longer ones ("huge"): the segmented radix sort
constexpr uint32_t kLdsSeg = 2048;

// Exclusive scan of the per-query row counts (n = queries + 1 entries, the
// last one 0) into u64 segment offsets, reduce-then-scan over tiles of
// kScanTile: no inter-block waiting, so it keeps its pace next to the
// persistent search kernels. The tile pass also lists the long segments
// (> kMediumSeg rows; one global atomic per tile).
constexpr uint32_t kScanTile = 4096;

// exclusive scan of one value per thread over a 256-thread block
__device__ __forceinline__ uint64_t blockExclusiveScan(uint64_t v, uint64_t& total, uint64_t* wsum) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint64_t pre = 0;
    total = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint64_t t = wsum[i];
        pre += i < w ? t : 0;
        total += t;
    }
    __syncthreads();
    return pre + x - v;
}

__global__ __launch_bounds__(256) void kTileSums(const uint32_t* __restrict__ cnt, uint32_t n,
                                                uint64_t* __restrict__ partial) {
    __shared__ uint64_t wsum[4];
    const uint32_t base = blockIdx.x * kScanTile;
    uint64_t acc = 0;
    for (uint32_t i = threadIdx.x; i < kScanTile && base + i < n; i += 256) acc += cnt[base + i];
    for (uint32_t off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void kScanPartials(uint64_t* __restrict__ partial, uint32_t ntiles) {
    __shared__ uint64_t wsum[4];
    uint64_t carry = 0;
    for (uint32_t b = 0; b < ntiles; b += 256) {
        const uint32_t i = b + threadIdx.x;
        const uint64_t v = i < ntiles ? partial[i] : 0;
        uint64_t tot;
        const uint64_t ex = blockExclusiveScan(v, tot, wsum);
        if (i < ntiles) partial[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(256) void kScanTiles(uint32_t* __restrict__ cnt, uint32_t n,
                                                 const uint64_t* __restrict__ partial, uint64_t* __restrict__ off,
                                                 uint32_t* __restrict__ list, uint32_t* __restrict__ nlist,
                                                 uint32_t* __restrict__ huge, uint32_t* __restrict__ nhuge) {
    __shared__ uint64_t wsum[4];
    __shared__ uint32_t llist[kScanTile];
    __shared__ uint32_t lcnt, lbase;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) lcnt = 0;
    const uint32_t base = blockIdx.x * kScanTile;
    uint64_t carry = partial[blockIdx.x];
    for (uint32_t c = 0; c < kScanTile; c += 256) {  // uniform trip count: block scans inside
        const uint32_t i = base + c + threadIdx.x;
        const uint32_t v = i < n ? cnt[i] : 0u;
        if (v) cnt[i] = 0u;  // zero again for the next batch
        uint64_t tot;
        const uint64_t ex = blockExclusiveScan(v, tot, wsum);
        if (i < n) off[i] = carry + ex;
        carry += tot;
        const uint64_t m = __ballot(v > kMediumSeg);
        if (m) {
            uint32_t wb = 0;
            const int leader = __ffsll((long long)m) - 1;
            if ((int)lane == leader) wb = atomicAdd(&lcnt, (uint32_t)__popcll(m));
            wb = __shfl(wb, leader);
            if (v > kMediumSeg) llist[wb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
            if (v > kLdsSeg) huge[atomicAdd(nhuge, 1u)] = i;  // rare: past the LDS sort (kSortBigLds)
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) lbase = lcnt ? atomicAdd(nlist, lcnt) : 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < lcnt; i += 256) list[lbase + i] = llist[i];
}

// One lane per reported cursor: locate every row of [lb, lb+len) into the
// query's segment [qoff[qid], qoff[qid+1]) of the key array (key = text
// position << 4 | e), from the slot the search kernel ranked it at (rank).
template <bool COUNT>
__global__ __launch_bounds__(256) void kLocate(LocateArgs a) {
    uint64_t steps = 0;
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < a.nhits;
         h += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 hit = a.hits[h];
        if (hit.z == 0) continue;  // reserved hole
        const uint64_t e = hit.w & 0xFu;
        const uint64_t out = a.qoff[hit.x] + a.rank[h];
        if (hit.w & kPosKnown) {  // resolved by the text phase, ranked where it was written
            a.keys[out] = ((uint64_t)hit.y << 4) | e;
            continue;
        }
        if (a.useSA) {  // full SA resident: one read per row
            for (uint32_t j = 0; j < hit.z; ++j) a.keys[out + j] = ((uint64_t)a.sa[hit.y + j] << 4) | e;
            continue;
        }
        for (uint32_t j = 0; j < hit.z; ++j) {  // fmc::LocateLinear: LF walk to a sample
            uint32_t row = hit.y + j;
            uint32_t st = 0;
            uint64_t gpos = 0;
            for (;;) {
                const uint4* q = reinterpret_cast<const uint4*>(a.occF + (row >> 6));
                const uint4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
                const uint32_t o = row & 63u;
                const uint64_t sampled = (uint64_t)a3.x | ((uint64_t)a3.y << 32);
                if ((sampled >> o) & 1ull) {
                    const uint32_t k = a1.y + (uint32_t)__popcll(sampled & lowMask(o));
                    gpos = (uint64_t)a.samples[k] + st;
                    break;
                }
                const uint64_t p[3] = {(uint64_t)a1.z | ((uint64_t)a1.w << 32),
                                       (uint64_t)a2.x | ((uint64_t)a2.y << 32),
                                       (uint64_t)a2.z | ((uint64_t)a2.w << 32)};
                const uint32_t c = symAt(p, o);
                if (c == 0 || st >= a.rate) {  // cannot happen on a well-formed index
                    atomicOr(a.flags, kFlagLocate);
                    break;
                }
                const uint32_t cnt[5] = {a0.x, a0.y, a0.z, a0.w, a1.x};
                row = a.C[c] + pick5(cnt, c - 1) + (uint32_t)__popcll(symMask(p, c) & lowMask(o));
                ++st;
            }
            if (COUNT) steps += st;
            a.keys[out + j] = (gpos << 4) | e;
        }
    }
    if (COUNT && steps) atomicAdd(a.counters, (unsigned long long)steps);
}

// What the sort kernels write per sorted key: the whole 24-B hit, or (COMPACT)
// the 8-B download record, batch-local query << 36 | key (text position << 4 | e).
template <bool COMPACT>
using SortOut = std::conditional_t<COMPACT, uint64_t, sahara_hit>;

__device__ __forceinline__ uint64_t compactRecord(uint64_t k, uint32_t localQuery) {
    return ((uint64_t)localQuery << 36) | k;
}

__device__ __forceinline__ void cswap(uint64_t& a, uint64_t& b) {
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// n <= kSmallSeg keys in a lane's registers (padded with ~0, which never
// moves): odd-even transposition, n rounds sort the n keys
__device__ __forceinline__ void sortSmall(uint64_t v[kSmallSeg], uint32_t n) {
#pragma unroll
    for (uint32_t r = 0; r < kSmallSeg; ++r) {
        if (r >= n) break;
#pragma unroll
        for (uint32_t i = r & 1u; i + 1 < kSmallSeg; i += 2) cswap(v[i], v[i + 1]);
    }
}

// <= 64 keys across a wave, one per lane (padded with ~0): bitonic over shuffles
__device__ __forceinline__ uint64_t sortWave(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint64_t o = __shfl_xor(v, j);
            const bool keepMin = ((lane & j) == 0) == ((lane & k) == 0);
            v = keepMin ? (v < o ? v : o) : (v < o ? o : v);
        }
    }
    return v;
}

// The two tiers a workgroup sorts itself, for thread t's segment of n keys at
// `at`: <= kSmallSeg in the lane's registers, <= kMediumSeg by the wave, one
// segment after the other. key(i) reads key i; sorted(i, k, owner) takes the
// sorted key k of place i, which belongs to the segment of thread `owner`.
// All lanes call it (wave-uniform).
template <typename At, typename Key, typename Sorted>
__device__ __forceinline__ void sortTiers(uint32_t n, At at, uint32_t t, Key key, Sorted sorted) {
    const uint32_t lane = t & 63u;
    if (n && n <= kSmallSeg) {
        uint64_t v[kSmallSeg];
#pragma unroll
        for (uint32_t i = 0; i < kSmallSeg; ++i) v[i] = i < n ? key(at + i) : ~0ull;
        sortSmall(v, n);
#pragma unroll
        for (uint32_t i = 0; i < kSmallSeg; ++i)
            if (i < n) sorted(at + i, v[i], t);
    }
    uint64_t med = __ballot(n > kSmallSeg && n <= kMediumSeg);
    while (med) {
        const int src = __ffsll((long long)med) - 1;
        med &= med - 1;
        const uint32_t sn = (uint32_t)__shfl((int)n, src);
        const At sat = __shfl(at, src);
        const uint64_t v = sortWave(lane < sn ? key(sat + lane) : ~0ull, lane);
        if (lane < sn) sorted(sat + lane, v, (t & ~63u) + (uint32_t)src);
    }
}

// Sort + decode, one workgroup per 256 consecutive queries. Their segments
// are one contiguous key range; when it fits kTileKeys (the common case: ~1.3
// rows per query) it is staged in LDS by coalesced loads, every segment is
// sorted there (sortTiers), and the decoded hits leave as one coalesced run of
// 24-B records. Long segments are left to kSortBigLds / the segmented radix
// sort (kDecodeBig). Record starts sit in LDS for texts of <= kLdsStarts
// records, so a decode's binary search waits on no global loads. A range
// larger than the tile takes the same tiers straight from global memory.
constexpr uint32_t kTileKeys = 1024;
constexpr uint16_t kSkipRow = 0xFFFFu;

// COMPACT: the hits leave as sahara_gpu_search's 8-B download records instead
// (kCompactHits' form: batch-local query << 36 | key), which is the sorted key
// with the query in front: no decode, and no record starts are read or staged.
template <bool COMPACT>
__global__ __launch_bounds__(256) void kSortDecode(const uint64_t* __restrict__ keys,
                                                  const uint64_t* __restrict__ qoff, uint32_t nq, uint64_t qidBase,
                                                  const uint64_t* __restrict__ starts, uint32_t nrec,
                                                  SortOut<COMPACT>* __restrict__ out) {
    __shared__ uint64_t sk[kTileKeys];
    __shared__ uint64_t soff[257];
    __shared__ uint64_t sst[COMPACT ? 1 : kLdsStarts];
    __shared__ uint16_t sq[kTileKeys];
    const uint32_t t = threadIdx.x;
    const bool ldsStarts = !COMPACT && nrec <= kLdsStarts;
    if (ldsStarts)
        for (uint32_t i = t; i < nrec; i += 256) sst[i] = starts[i];
    // sorted key k of the batch's query lq -> out[i]
    auto put = [&](uint64_t i, uint64_t k, uint32_t lq) {
        if constexpr (COMPACT) out[i] = compactRecord(k, lq);
        else out[i] = ldsStarts ? decodeKey(k, qidBase + lq, sst, nrec) : decodeKey(k, qidBase + lq, starts, nrec);
    };
    for (uint32_t q0 = blockIdx.x * 256u; q0 < nq; q0 += gridDim.x * 256u) {
        const uint32_t q = q0 + t;
        soff[t] = qoff[q < nq ? q : nq];
        if (t == 0) soff[256] = qoff[q0 + 256u < nq ? q0 + 256u : nq];
        __syncthreads();
        const uint64_t base = soff[0], R = soff[256] - base;
        const uint64_t b = soff[t];
        const uint32_t n = q < nq ? (uint32_t)(soff[t + 1] - b) : 0u;
        if (R <= kTileKeys) {  // block-uniform: sorted in the tile, each key's query noted beside it
            for (uint32_t i = t; i < (uint32_t)R; i += 256) sk[i] = keys[base + i];
            __syncthreads();
            const uint32_t lb = (uint32_t)(b - base);
            sortTiers(n, lb, t, [&](uint32_t i) { return sk[i]; },
                      [&](uint32_t i, uint64_t k, uint32_t owner) { sk[i] = k; sq[i] = (uint16_t)owner; });
            if (n > kMediumSeg)
                for (uint32_t i = 0; i < n; ++i) sq[lb + i] = kSkipRow;  // the long-segment kernels decode it
            __syncthreads();
            for (uint32_t i = t; i < (uint32_t)R; i += 256) {
                const uint32_t lq = sq[i];
                if (lq != kSkipRow) put(base + i, sk[i], q0 + lq);
            }
            __syncthreads();  // soff, sk, sq are reused by the next range
            continue;
        }
        __syncthreads();  // soff is reused by the next range
        sortTiers(n, b, t, [&](uint64_t i) { return keys[i]; },
                  [&](uint64_t i, uint64_t k, uint32_t owner) { put(i, k, q0 + owner); });
    }
}

// One workgroup per long segment (already sorted): decode.
template <bool COMPACT>
__global__ __launch_bounds__(256) void kDecodeBig(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ qoff,
                                                 const uint32_t* __restrict__ big, uint32_t nbig, uint64_t qidBase,
                                                 const uint64_t* __restrict__ starts, uint32_t nrec,
                                                 SortOut<COMPACT>* __restrict__ out) {
    for (uint32_t s = blockIdx.x; s < nbig; s += gridDim.x) {
        const uint32_t q = big[s];
        const uint64_t b = qoff[q], e = qoff[q + 1];
        for (uint64_t i = b + threadIdx.x; i < e; i += blockDim.x) {
            if constexpr (COMPACT) out[i] = compactRecord(keys[i], q);
            else out[i] = decodeKey(keys[i], qidBase + q, starts, nrec);
        }
    }
}

// Long segments (kMediumSeg < rows <= kLdsSeg): one workgroup per segment,
// keys padded to a power of two with ~0 in LDS, bitonic sort, decoded hits
// written in order. 16 KB of LDS and no scratch in HBM: it fits beside the
// text phase's workgroups, where rocPRIM's segmented radix sort (whose blocks
// need more LDS than the text phase leaves free) waited for the text launch
// to drain, up to 1.3 ms per batch at C3 (profiles/r03_v5_c3_timeline.txt).
template <bool COMPACT>
__global__ __launch_bounds__(256) void kSortBigLds(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ qoff,
                                                  const uint32_t* __restrict__ big, uint32_t nbig, uint64_t qidBase,
                                                  const uint64_t* __restrict__ starts, uint32_t nrec,
                                                  SortOut<COMPACT>* __restrict__ out) {
    __shared__ uint64_t K[kLdsSeg];
    for (uint32_t s = blockIdx.x; s < nbig; s += gridDim.x) {
        const uint32_t q = big[s];
        const uint64_t b = qoff[q], e = qoff[q + 1];
        const uint32_t n = (uint32_t)(e - b);
        if (n > kLdsSeg) continue;  // a huge segment: the radix sort path (block-uniform)
        uint32_t P = 1;
        while (P < n) P <<= 1;
        for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) K[i] = i < n ? keys[b + i] : ~0ull;
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const uint64_t x = K[i], y = K[p];
                        const bool up = (i & k) == 0;
                        if ((x > y) == up) {
                            K[i] = y;
                            K[p] = x;
                        }
                    }
                }
                __syncthreads();
            }
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            if constexpr (COMPACT) out[b + i] = compactRecord(K[i], q);
            else out[b + i] = decodeKey(K[i], qidBase + q, starts, nrec);
        }
        __syncthreads();
    }
}

struct SegOff {  // begin (d = 0) / end (d = 1) of a listed query's segment
    const uint64_t* qoff;
    uint32_t d;
    __host__ __device__ uint32_t operator()(const uint32_t& q) const { return (uint32_t)qoff[q + d]; }
};

}  // namespace

void querySegments(uint32_t* qcnt, uint32_t nq, uint64_t* qoff, uint64_t* partial, uint32_t* big, uint32_t* nbig,
                   uint32_t* huge, uint32_t* nhuge, hipStream_t st) {
    // qcnt[nq] stays 0, so qoff[nq] = total rows
    const uint32_t n = nq + 1, tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(kTileSums, dim3(tiles), dim3(256), 0, st, qcnt, n, partial);
    hipLaunchKernelGGL(kScanPartials, dim3(1), dim3(256), 0, st, partial, tiles);
    hipLaunchKernelGGL(kScanTiles, dim3(tiles), dim3(256), 0, st, qcnt, n, partial, qoff, big, nbig, huge, nhuge);
    SH_HIP(hipGetLastError());
}

uint32_t scanTiles(uint32_t nq) { return (nq + 1 + kScanTile - 1) / kScanTile; }

// ... and clears what it has read, with the slot's queue counters: nothing on
// the device reads them again before the slot's next batch, so the slot is
// reset here and not by fills of its own further down the chain.
__global__ void kBatchTotals(uint32_t* __restrict__ small, uint32_t* __restrict__ queues,
                             const uint64_t* __restrict__ rowTotal, uint32_t* __restrict__ segCounts,
                             uint32_t* __restrict__ out) {
    const uint32_t i = threadIdx.x;
    if (i < kSlotWords) {
        out[i] = small[i];
        small[i] = 0;
    } else if (i < 10) {
        out[i] = (uint32_t)(*rowTotal >> (32 * (i - 8)));
    } else if (i < 12) {
        out[i] = segCounts[i - 10];
        segCounts[i - 10] = 0;
    }
    for (uint32_t w = i; w < kQueuesWords; w += blockDim.x) queues[w] = 0;
}

__global__ void kRoundReset(uint32_t* __restrict__ small, uint32_t* __restrict__ queues) {
    if (threadIdx.x == 0) {
        small[kSwRoundTasks] = small[kSwTaskCount];
        small[kSwSeedCount] = 0;
    }
    for (uint32_t w = threadIdx.x; w < kQueuesWords; w += blockDim.x) queues[w] = 0;
}

void launchRoundReset(uint32_t* small, uint32_t* queues, hipStream_t st) {
    hipLaunchKernelGGL(kRoundReset, dim3(1), dim3(256), 0, st, small, queues);
    SH_HIP(hipGetLastError());
}

void launchBatchTotals(uint32_t* small, uint32_t* queues, const uint64_t* rowTotal, uint32_t* segCounts, uint32_t* out,
                       hipStream_t st) {
    hipLaunchKernelGGL(kBatchTotals, dim3(1), dim3(64), 0, st, small, queues, rowTotal, segCounts, out);
    SH_HIP(hipGetLastError());
}

// The locate chain's flags word into the batch's record in pinned host memory,
// cleared for the next batch's chain.
__global__ void kLocateFlagsOut(uint32_t* __restrict__ flags, uint32_t* __restrict__ out) {
    *out = *flags;
    *flags = 0;
}

void launchLocateFlagsOut(uint32_t* flags, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(kLocateFlagsOut, dim3(1), dim3(1), 0, st, flags, out);
    SH_HIP(hipGetLastError());
}

void launchLocate(const LocateArgs& a, bool count, hipStream_t st) {
    if (a.nhits == 0) return;
    const uint64_t blocks = std::min<uint64_t>((a.nhits + 255) / 256, 65536);
    if (count) hipLaunchKernelGGL(kLocate<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else       hipLaunchKernelGGL(kLocate<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    SH_HIP(hipGetLastError());
}

size_t bigSortTempBytes(uint64_t rows, uint32_t nbig) {
    size_t tb = 0;
    rocprim::transform_iterator<const uint32_t*, SegOff, uint32_t> bi(nullptr, SegOff{nullptr, 0});
    rocprim::transform_iterator<const uint32_t*, SegOff, uint32_t> ei(nullptr, SegOff{nullptr, 1});
    SH_HIP(rocprim::segmented_radix_sort_keys(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (unsigned)rows, nbig, bi, ei, 0, 36, (hipStream_t)0));
    return tb;
}

template <bool COMPACT>
static void sortInto(uint64_t* k0, uint64_t* k1, uint64_t rows, const uint64_t* qoff, uint32_t nq, const uint32_t* big,
                     uint32_t nbig, const uint32_t* huge, uint32_t nhuge, uint64_t qidBase, const uint64_t* starts,
                     uint32_t nrec, SortOut<COMPACT>* out, void* tmp, size_t tmpBytes, hipStream_t st) {
    if (rows == 0) return;
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>((nq + 255) / 256, 65536));
    hipLaunchKernelGGL(kSortDecode<COMPACT>, dim3(blocks), dim3(256), 0, st, k0, qoff, nq, qidBase, starts, nrec, out);
    SH_HIP(hipGetLastError());
    if (nbig) {  // long segments in LDS; huge ones skipped there
        hipLaunchKernelGGL(kSortBigLds<COMPACT>, dim3(std::min<uint32_t>(nbig, 4096)), dim3(256), 0, st, k0, qoff, big,
                           nbig, qidBase, starts, nrec, out);
        SH_HIP(hipGetLastError());
    }
    if (nhuge == 0) return;
    rocprim::transform_iterator<const uint32_t*, SegOff, uint32_t> bi(huge, SegOff{qoff, 0});
    rocprim::transform_iterator<const uint32_t*, SegOff, uint32_t> ei(huge, SegOff{qoff, 1});
    size_t tb = tmpBytes;
    SH_HIP(rocprim::segmented_radix_sort_keys(tmp, tb, (const uint64_t*)k0, k1, (unsigned)rows, nhuge, bi, ei, 0, 36,
                                              st));
    hipLaunchKernelGGL(kDecodeBig<COMPACT>, dim3(std::min<uint32_t>(nhuge, 65536)), dim3(256), 0, st, k1, qoff, huge,
                       nhuge, qidBase, starts, nrec, out);
    SH_HIP(hipGetLastError());
}

void sortDecode(uint64_t* k0, uint64_t* k1, uint64_t rows, const uint64_t* qoff, uint32_t nq, const uint32_t* big,
                uint32_t nbig, const uint32_t* huge, uint32_t nhuge, uint64_t qidBase, const uint64_t* starts,
                uint32_t nrec, sahara_hit* out, void* tmp, size_t tmpBytes, hipStream_t st) {
    sortInto<false>(k0, k1, rows, qoff, nq, big, nbig, huge, nhuge, qidBase, starts, nrec, out, tmp, tmpBytes, st);
}

void sortCompact(uint64_t* k0, uint64_t* k1, uint64_t rows, const uint64_t* qoff, uint32_t nq, const uint32_t* big,
                 uint32_t nbig, const uint32_t* huge, uint32_t nhuge, uint64_t* out, void* tmp, size_t tmpBytes,
                 hipStream_t st) {
    sortInto<true>(k0, k1, rows, qoff, nq, big, nbig, huge, nhuge, 0, nullptr, 0, out, tmp, tmpBytes, st);
}

}  // namespace sahara
