// hits.hip — what happens to a batch's hit records after the sort: digest,
// copies with shifted ids, the multi-part merge by query, --max_hits on the
// device with what the batch's stages share (replaceBatch, scanFlagsCount),
// and the compact 8-B download records and their way back (gfx950).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "search_device.h"

namespace sahara {
namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__global__ void kDigest(const sahara_hit* __restrict__ h, uint64_t n, unsigned long long* out) {
    uint64_t acc = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x)
        acc += mix64(h[i].qid * 0x9E3779B97F4A7C15ull ^ mix64(((uint64_t)h[i].seq_id << 40) ^ (h[i].pos << 4) ^ h[i].err));
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, (unsigned long long)acc);
}

// Hit records into a caller's device buffer with qids shifted by qidOffset
// (rank-local -> global qids before a gather across ranks).
__global__ void kCopyHits(const sahara_hit* __restrict__ h, uint64_t n, uint64_t qidOffset,
                          sahara_hit* __restrict__ dst) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        sahara_hit r = h[i];
        r.qid += qidOffset;
        dst[i] = r;
    }
}

}  // namespace

// Multi-part index (capi.cpp run): a part's hits with its first global
// record id added to seq_id, appended to the hits of the parts before it.
__global__ void kOffsetSeq(const sahara_hit* __restrict__ in, uint64_t n, uint32_t rec0, sahara_hit* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        sahara_hit h = in[i];
        h.seq_id += rec0;
        out[i] = h;
    }
}

void launchOffsetSeq(const sahara_hit* in, uint64_t n, uint64_t rec0, sahara_hit* out, hipStream_t st) {
    if (n == 0) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(kOffsetSeq, dim3((unsigned)blocks), dim3(256), 0, st, in, n, (uint32_t)rec0, out);
    SH_HIP(hipGetLastError());
}

__global__ void kQidKeys(const sahara_hit* __restrict__ h, uint64_t n, uint64_t* __restrict__ key,
                         uint32_t* __restrict__ idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        key[i] = h[i].qid;
        idx[i] = (uint32_t)i;
    }
}

__global__ void kGatherHits(const sahara_hit* __restrict__ in, const uint32_t* __restrict__ idx, uint64_t n,
                            sahara_hit* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = in[idx[i]];
}

// --max_hits n on the device (search_n, search.cpp:228,231; the policy U6 of
// include/sahara_hip.h): per query, of its hits in canonical order, the n
// distinct (seq_id, pos) with the fewest errors (each once, with its minimum
// e: the first of its run), ties by (seq_id, pos). One thread per query: the
// plan counts the distinct positions per error count and fixes the error
// threshold e* and how many at e* are kept (quota); the write keeps, in
// order, every first-of-run below e* and the first `quota` at e*.
struct LimitPlan { uint32_t eStar, quota, kept; };
__device__ __forceinline__ LimitPlan limitPlan(const sahara_hit* __restrict__ h, uint64_t b, uint64_t e, uint32_t n) {
    uint32_t hist[16];
#pragma unroll
    for (uint32_t x = 0; x < 16; ++x) hist[x] = 0;
    uint32_t distinct = 0, ps = 0xFFFFFFFFu;
    uint64_t pp = ~0ull;
    for (uint64_t i = b; i < e; ++i) {
        const sahara_hit x = h[i];
        if (x.seq_id != ps || x.pos != pp) {
            ++distinct;
#pragma unroll
            for (uint32_t v = 0; v < 16; ++v) hist[v] += x.err == v ? 1u : 0u;
            ps = x.seq_id;
            pp = x.pos;
        }
    }
    if (distinct <= n) return {16u, 0u, distinct};
    uint32_t cum = 0;
#pragma unroll
    for (uint32_t v = 0; v < 16; ++v) {
        if (cum < n && cum + hist[v] >= n) return {v, n - cum, n};
        cum += hist[v];
    }
    return {16u, 0u, distinct};  // unreachable: the histogram sums to distinct > n
}

__global__ void kLimitCount(const sahara_hit* __restrict__ h, const uint64_t* __restrict__ qoff, uint32_t nq,
                            uint32_t n, uint32_t* __restrict__ kcnt) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q <= nq; q += gridDim.x * blockDim.x)
        kcnt[q] = q < nq ? limitPlan(h, qoff[q], qoff[q + 1], n).kept : 0u;
}

__global__ void kLimitWrite(const sahara_hit* __restrict__ h, const uint64_t* __restrict__ qoff, uint32_t nq,
                            uint32_t n, const uint64_t* __restrict__ koff, sahara_hit* __restrict__ dst) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
        const uint64_t b = qoff[q], e = qoff[q + 1];
        const LimitPlan P = limitPlan(h, b, e, n);
        uint64_t w = koff[q];
        uint32_t used = 0, ps = 0xFFFFFFFFu;
        uint64_t pp = ~0ull;
        for (uint64_t i = b; i < e; ++i) {
            const sahara_hit x = h[i];
            if (x.seq_id == ps && x.pos == pp) continue;
            ps = x.seq_id;
            pp = x.pos;
            const bool keep = x.err < P.eStar || (x.err == P.eStar && used < P.quota);
            used += x.err == P.eStar && keep ? 1u : 0u;
            if (keep) dst[w++] = x;
        }
    }
}

// Applies --max_hits n to the batch in place, the last of its stages
// (search.h BatchView). Host-synchronous: the kept total comes back through
// v.kept.
void limitBatch(BatchView& v, uint32_t n, LimitBufs& B) {
    if (v.rows == 0 || v.nq == 0) return;
    const uint32_t nq = v.nq;
    B.cnt.reserve((size_t)nq + 1);
    B.off.reserve((size_t)nq + 1);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>((nq + 256) / 256, 16384));
    hipLaunchKernelGGL(kLimitCount, dim3(blocks), dim3(256), 0, v.st, v.hits, v.qoff, nq, n, B.cnt.ptr);
    SH_HIP(hipGetLastError());
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::exclusive_scan(temp, bytes, B.cnt.ptr, B.off.ptr, (uint64_t)0, (size_t)nq + 1,
                                       rocprim::plus<uint64_t>(), v.st);
    });
    SH_HIP(hipMemcpyAsync(v.kept, B.off.ptr + nq, 8, hipMemcpyDeviceToHost, v.st));
    SH_HIP(hipStreamSynchronize(v.st));
    const uint64_t kept = *v.kept;
    if (kept == v.rows) return;  // nothing to drop in this batch
    v.scratch.reserve(std::max<uint64_t>(kept, 1));
    hipLaunchKernelGGL(kLimitWrite, dim3(blocks), dim3(256), 0, v.st, v.hits, v.qoff, nq, n, B.off.ptr, v.scratch.ptr);
    SH_HIP(hipGetLastError());
    replaceBatch(v, kept);
}

namespace {

// The per-query segments of n sorted records: qoff[q] = the first of them
// whose qid is not below qidBase + q, qoff[nq] = n. One binary search per query.
__global__ void kLociSegments(const sahara_hit* __restrict__ h, uint64_t loci, uint64_t qidBase, uint32_t nq,
                              uint64_t* __restrict__ qoff) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q <= nq; q += gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = loci;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (h[mid].qid < qidBase + q) lo = mid + 1;
            else hi = mid;
        }
        qoff[q] = lo;
    }
}

}  // namespace

void replaceBatch(BatchView& v, uint64_t n) {
    if (n) SH_HIP(hipMemcpyAsync(v.hits, v.scratch.ptr, n * sizeof(sahara_hit), hipMemcpyDeviceToDevice, v.st));
    v.rows = n;
    if (!v.later) return;
    const uint32_t qblocks = std::min<uint32_t>(v.nq / 256 + 1, 16384);
    hipLaunchKernelGGL(kLociSegments, dim3(qblocks), dim3(256), 0, v.st, v.hits, n, v.q0, v.nq, v.qoff);
    SH_HIP(hipGetLastError());
}

uint64_t scanFlagsCount(uint32_t* flag, uint32_t* num, BatchView& v) {
    withTemp(v.tmp, [&](void* temp, size_t& bytes) {
        return rocprim::inclusive_scan(temp, bytes, flag, num, (size_t)v.rows, rocprim::plus<uint32_t>(), v.st);
    });
    *v.kept = 0;  // (the count is 32 bits: the low half of the word)
    SH_HIP(hipMemcpyAsync(v.kept, num + (v.rows - 1), 4, hipMemcpyDeviceToHost, v.st));
    SH_HIP(hipStreamSynchronize(v.st));
    return *v.kept;
}

// Stable sort of hit records by qid (rocPRIM's LSD radix sort is stable):
// the parts' hits, each part in canonical order and every part's records
// after the previous part's, come out in canonical (qid, seq_id, pos, err)
// order. Only the bits of qids below nqid are sorted; the key / index
// buffers (B) are the context's, reused across calls.
void sortHitsByQid(const sahara_hit* in, uint64_t n, uint64_t nqid, sahara_hit* out, MergeBufs& B, DevBuf<char>& tmp,
                   hipStream_t st) {
    if (n == 0) return;
    if (n >= (1ull << 32)) throw Error("more than 2^32 hits to merge across index parts");
    B.k0.reserve(n);
    B.k1.reserve(n);
    B.v0.reserve(n);
    B.v1.reserve(n);
    unsigned endBit = 1;
    while (endBit < 64 && (nqid > (1ull << endBit))) ++endBit;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(kQidKeys, dim3((unsigned)blocks), dim3(256), 0, st, in, n, B.k0.ptr, B.v0.ptr);
    SH_HIP(hipGetLastError());
    withTemp(tmp, [&](void* temp, size_t& bytes) {
        return rocprim::radix_sort_pairs(temp, bytes, B.k0.ptr, B.k1.ptr, B.v0.ptr, B.v1.ptr, (size_t)n, 0, endBit, st);
    });
    hipLaunchKernelGGL(kGatherHits, dim3((unsigned)blocks), dim3(256), 0, st, in, B.v1.ptr, n, out);
    SH_HIP(hipGetLastError());
    SH_HIP(hipStreamSynchronize(st));
}

// sahara_gpu_search's download form of a batch's hits, 8 B instead of 24:
// (qid - qidBase) << 36 | text position << 4 | e (batches < 2^28 queries,
// texts < 2^32, e < 16), expanded back on the host (capi.cpp expandHits).
__global__ void kCompactHits(const sahara_hit* __restrict__ h, uint64_t n, uint64_t qidBase,
                             const uint64_t* __restrict__ starts, uint64_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const sahara_hit x = h[i];
        out[i] = ((x.qid - qidBase) << 36) | ((starts[x.seq_id] + x.pos) << 4) | x.err;
    }
}

// The way back, for a batch that the sort wrote as compact records only:
// record i -> whole hit i (qid = qidBase + its batch-local query). Record
// starts in LDS for texts of <= kLdsStarts records, as in kSortDecode.
__global__ __launch_bounds__(256) void kExpandRecs(const uint64_t* __restrict__ recs, uint64_t n, uint64_t qidBase,
                                                  const uint64_t* __restrict__ starts, uint32_t nrec,
                                                  sahara_hit* __restrict__ out) {
    __shared__ uint64_t sst[kLdsStarts];
    const bool ldsStarts = nrec <= kLdsStarts;  // block-uniform
    if (ldsStarts) {
        for (uint32_t i = threadIdx.x; i < nrec; i += blockDim.x) sst[i] = starts[i];
        __syncthreads();
    }
    const uint64_t* const st = ldsStarts ? sst : starts;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = recs[i];
        out[i] = decodeKey(v & ((1ull << 36) - 1), qidBase + (v >> 36), st, nrec);
    }
}

void launchExpandRecs(const uint64_t* recs, uint64_t n, uint64_t qidBase, const uint64_t* starts, uint32_t nrec,
                      sahara_hit* out, hipStream_t st) {
    if (n == 0) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(kExpandRecs, dim3((unsigned)blocks), dim3(256), 0, st, recs, n, qidBase, starts, nrec, out);
    SH_HIP(hipGetLastError());
}

// `out` may be page-locked host memory: then the kernel's stores are the
// PCIe transfer (posted writes, ~link rate), and a few workgroups (maxBlocks)
// keep it off most CUs.
void launchCompactHits(const sahara_hit* h, uint64_t n, uint64_t qidBase, const uint64_t* starts, uint64_t* out,
                       hipStream_t st, uint32_t maxBlocks) {
    if (n == 0) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, std::max<uint32_t>(maxBlocks, 1));
    hipLaunchKernelGGL(kCompactHits, dim3((unsigned)blocks), dim3(256), 0, st, h, n, qidBase, starts, out);
    SH_HIP(hipGetLastError());
}

void launchDigest(const sahara_hit* h, uint64_t n, unsigned long long* out, hipStream_t st) {
    if (n == 0) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(kDigest, dim3((unsigned)blocks), dim3(256), 0, st, h, n, out);
    SH_HIP(hipGetLastError());
}

void launchCopyHits(const sahara_hit* h, uint64_t n, uint64_t qidOffset, sahara_hit* dst, hipStream_t st) {
    if (n == 0) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 16384);
    hipLaunchKernelGGL(kCopyHits, dim3((unsigned)blocks), dim3(256), 0, st, h, n, qidOffset, dst);
    SH_HIP(hipGetLastError());
}

}  // namespace sahara
