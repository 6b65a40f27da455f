// patterns.hip — the pattern packers: query symbols in their upload forms into
// the two forms the search reads, 4-bit words (FM phase) and 3-bit-plane
// blocks (text phase), and the reverse-complement interleave (gfx950).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "search_device.h"

namespace sahara {
namespace {

// pattern bytes (one symbol per byte) -> 4-bit words, patWords per pattern
// Also validates the ranks (ivs::verify_rank, search.cpp:118-120): *bad != 0
// if any is 0 or >= sigma.
__global__ void kPackPatterns(const uint8_t* __restrict__ src, uint64_t npat, uint32_t m, uint32_t patWords,
                              uint32_t sigma, uint32_t* __restrict__ dst, uint32_t* __restrict__ bad) {
    const uint64_t total = npat * patWords;
    bool invalid = false;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = i / patWords;
        const uint32_t w = (uint32_t)(i - p * patWords);
        uint32_t v = 0;
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t q = w * 8 + j;
            if (q < m) {
                const uint32_t r = src[p * m + q];
                invalid |= r == 0 || r >= sigma;
                v |= (r & 0xFu) << (4 * j);
            }
        }
        dst[i] = v;
    }
    if (__any(invalid) && (threadIdx.x & 63u) == 0) atomicOr(bad, 1u);
}

// pattern bytes -> 3-bit-plane blocks of 32 symbols (device_index.h),
// patBlocks per pattern, zero past m (the text phase's layout)
__global__ void kPackPatterns3(const uint8_t* __restrict__ src, uint64_t npat, uint32_t m, uint32_t patBlocks,
                               uint4* __restrict__ dst) {
    const uint64_t total = npat * patBlocks;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = i / patBlocks;
        const uint32_t b = (uint32_t)(i - p * patBlocks);
        uint32_t p0 = 0, p1 = 0, p2 = 0;
        for (uint32_t j = 0; j < 32; ++j) {
            const uint32_t q = b * 32 + j;
            if (q < m) {
                const uint32_t r = src[p * m + q];
                p0 |= (r & 1u) << j;
                p1 |= ((r >> 1) & 1u) << j;
                p2 |= ((r >> 2) & 1u) << j;
            }
        }
        dst[i] = make_uint4(p0, p1, p2, 0u);
    }
}

}  // namespace

// Host upload format -> one byte per symbol: byte i of `nib` holds symbols 2i
// (low nibble) and 2i + 1 (high nibble). A thread expands 8 bytes into 16.
__global__ void kUnpackNibbles(const uint8_t* __restrict__ nib, uint8_t* __restrict__ dst, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w * 16 < n; w += stride) {
        if (w * 16 + 16 <= n) {
            const uint64_t x = *reinterpret_cast<const uint64_t*>(nib + w * 8);
            uint32_t o[4];
            for (int q = 0; q < 4; ++q) {
                const uint32_t b = (uint32_t)(x >> (16 * q));   // two packed bytes -> four symbols
                o[q] = (b & 0xFu) | ((b >> 4) & 0xFu) << 8 | ((b >> 8) & 0xFu) << 16 | ((b >> 12) & 0xFu) << 24;
            }
            *reinterpret_cast<uint4*>(dst + w * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (uint64_t i = w * 16; i < n; ++i) dst[i] = (nib[i >> 1] >> ((i & 1) * 4)) & 0xFu;
        }
    }
}

void launchUnpackNibbles(const uint8_t* nib, uint8_t* dst, uint64_t n, hipStream_t st) {
    const uint64_t blocks = std::min<uint64_t>((n / 16 + 256) / 256, 65536);
    hipLaunchKernelGGL(kUnpackNibbles, dim3((unsigned)blocks), dim3(256), 0, st, nib, dst, n);
    SH_HIP(hipGetLastError());
}

// A streamed 2-bit chunk straight into the search's two pattern forms, with
// no byte pass: 4-bit words (FM phase) and 3-bit-plane blocks (text phase)
// of the patterns [p0, p1). Pattern p is row p, or (rc) read p / 2 and, for
// odd p, its reverse complement (search.cpp:121-123: reversed, codes
// complemented as c ^ 3); read r starts at chunk-local symbol so + (r - r0) * m
// (so < 4: reads given packed start anywhere in a byte).
// `exc` lists the chunk's N positions in ascending order (rank 4). One thread
// per (pattern, 32-symbol block): 64 bits of codes from three word loads,
// even / odd bits gathered into the code planes c0 / c1, then
//   rank bit 0 = ~c0 | c1 (dna5: T = 5) or ~c0 (dna4), bit 1 = c0 ^ c1,
//   bit 2 = c0 & c1, and N = 100.
__device__ __forceinline__ uint32_t evenBits(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (uint32_t)(x | (x >> 16));
}
__device__ __forceinline__ uint32_t spreadNibbles(uint32_t x) {  // bit j of 8 -> bit 4j
    x &= 0xFFu;
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    return (x | (x << 3)) & 0x11111111u;
}
__global__ void kPackFrom2(const uint8_t* __restrict__ src, uint32_t so, const uint32_t* __restrict__ exc,
                           uint32_t nExc, uint64_t r0, uint64_t p0, uint64_t p1, uint32_t m, uint32_t rc, uint32_t dna5,
                           uint32_t patWords, uint32_t patBlocks, uint32_t* __restrict__ pats,
                           uint4* __restrict__ pats3) {
    const uint64_t total = (p1 - p0) * patBlocks;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = p0 + i / patBlocks;
        const uint32_t b = (uint32_t)(i % patBlocks);
        const uint64_t r = rc ? p >> 1 : p;
        const bool rev = rc && (p & 1u);
        const uint32_t nsym = min(32u, m - 32u * b);
        const uint64_t start = so + (r - r0) * m + (rev ? m - 32u * b - nsym : 32u * b);  // source symbols [start, start + nsym)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(src + (start >> 4) * 4);
        const uint32_t sh = (uint32_t)(start & 15u) * 2u;
        uint64_t v = ((uint64_t)w[1] << 32) | w[0];
        if (sh) v = (v >> sh) | ((uint64_t)w[2] << (64u - sh));
        uint32_t c0 = evenBits(v), c1 = evenBits(v >> 1);
        const uint32_t valid = nsym >= 32u ? 0xFFFFFFFFu : (1u << nsym) - 1u;
        uint32_t nm = 0;
        if (nExc) {
            uint32_t lo = 0, hi = nExc;  // first listed N at or after start
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (exc[mid] < start) lo = mid + 1; else hi = mid;
            }
            for (; lo < nExc && exc[lo] < start + nsym; ++lo) nm |= 1u << (uint32_t)(exc[lo] - start);
        }
        if (rev) {  // symbol q = complement of source symbol nsym - 1 - q
            c0 = ~__builtin_bitreverse32(c0) >> (32u - nsym);
            c1 = ~__builtin_bitreverse32(c1) >> (32u - nsym);
            nm = __builtin_bitreverse32(nm) >> (32u - nsym);
        }
        const uint32_t P0 = ((dna5 ? (~c0 | c1) : ~c0) & ~nm) & valid;
        const uint32_t P1 = ((c0 ^ c1) & ~nm) & valid;
        const uint32_t P2 = ((c0 & c1) | nm) & valid;
        pats3[p * patBlocks + b] = make_uint4(P0, P1, P2, 0u);
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t wi = 4u * b + t;
            if (wi < patWords)
                pats[p * patWords + wi] = spreadNibbles(P0 >> (8 * t)) | (spreadNibbles(P1 >> (8 * t)) << 1) |
                                          (spreadNibbles(P2 >> (8 * t)) << 2);
        }
    }
}

void launchPackFrom2(const uint8_t* src, uint32_t so, const uint32_t* exc, uint32_t nExc, uint64_t r0, uint64_t p0,
                     uint64_t p1, uint32_t m, bool rc, uint32_t sigma, uint32_t patWords, uint32_t patBlocks,
                     uint32_t* pats, uint4* pats3, hipStream_t st) {
    const uint64_t total = (p1 - p0) * patBlocks;
    if (total == 0) return;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(kPackFrom2, dim3((unsigned)blocks), dim3(256), 0, st, src, so, exc, nExc, r0, p0, p1, m,
                       rc ? 1u : 0u, sigma == 6 ? 1u : 0u, patWords, patBlocks, pats, pats3);
    SH_HIP(hipGetLastError());
}

// Query ingest's reverse-complement interleave (search.cpp:121-127) on the
// device: pattern 2r = read r, 2r + 1 = its reverse complement (A<->T, C<->G,
// N->N; ivs::reverse_complement_rank), for the patterns [2 * r0, pEnd) of the
// reads [r0, r1). One wave per read: lane j copies symbol j and writes its
// complement to position m - 1 - j of the next pattern (coalesced bytes).
__global__ void kInterleaveRC(const uint8_t* __restrict__ reads, uint64_t r0, uint64_t r1, uint32_t m,
                              uint32_t sigma, uint64_t pEnd, uint8_t* __restrict__ pats) {
    const uint32_t comp = sigma == 6 ? 0x142350u : 0x12340u;  // nibble c: complement of rank c (0 past sigma)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
    for (uint64_t r = r0 + (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; r < r1; r += waves) {
        const uint8_t* src = reads + r * m;
        uint8_t* fwd = pats + 2 * r * m;
        uint8_t* rev = fwd + m;
        const bool withRev = 2 * r + 1 < pEnd;
        for (uint32_t j = lane; j < m; j += 64) {
            const uint32_t s = src[j];
            fwd[j] = (uint8_t)s;
            if (withRev) rev[m - 1 - j] = s < 8 ? (uint8_t)((comp >> (4 * s)) & 0xFu) : (uint8_t)0;
        }
    }
}

void launchInterleaveRC(const uint8_t* reads, uint64_t r0, uint64_t r1, uint32_t m, uint32_t sigma, uint64_t pEnd,
                        uint8_t* pats, hipStream_t st) {
    r1 = std::min(r1, (pEnd + 1) / 2);  // reads whose forward pattern is within the limit
    if (r1 <= r0) return;
    const uint64_t blocks = std::min<uint64_t>((r1 - r0 + 3) / 4, 65536);
    hipLaunchKernelGGL(kInterleaveRC, dim3((unsigned)blocks), dim3(256), 0, st, reads, r0, r1, m, sigma, pEnd, pats);
    SH_HIP(hipGetLastError());
}

void launchPackPatterns(const uint8_t* src, uint64_t npat, uint32_t m, uint32_t patWords, uint32_t sigma,
                        uint32_t* dst, uint32_t* bad, hipStream_t st) {
    const uint64_t blocks = std::min<uint64_t>((npat * patWords + 255) / 256, 65536);
    hipLaunchKernelGGL(kPackPatterns, dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(256), 0, st, src, npat, m,
                       patWords, sigma, dst, bad);
    SH_HIP(hipGetLastError());
}

void launchPackPatterns3(const uint8_t* src, uint64_t npat, uint32_t m, uint32_t patBlocks, uint4* dst,
                         hipStream_t st) {
    const uint64_t blocks = std::min<uint64_t>((npat * patBlocks + 255) / 256, 65536);
    hipLaunchKernelGGL(kPackPatterns3, dim3((unsigned)blocks), dim3(256), 0, st, src, npat, m, patBlocks, dst);
    SH_HIP(hipGetLastError());
}

}  // namespace sahara
