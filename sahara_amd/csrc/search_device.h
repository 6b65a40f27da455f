// search_device.h — device-side pieces that the kernel units (search_fm.hip,
// search_text.hip, locate_sort.hip, hits.hip and the stage files) share:
// global-memory accesses that say so, the per-wave slot reservation of the
// append-only outputs, the striped work queue, the plan of an in-wave steal,
// the decode of a sorted key and the canonical order of hit records.
#pragma once
#include <hip/hip_runtime.h>

#include "search.h"

namespace sahara {
namespace {

// Pointers that come from memory (the slot table), from integers (Occ line
// addresses) or that may point to LDS or global memory (a stack level) are
// generic: accesses through them are flat instructions, which also count
// against the LDS counter and make every LDS wait wait for them (and a flat
// access of LDS is slower than a ds_ one). Where they address global memory,
// say so. (The host pass of a kernel file parses kernel bodies too, where
// class types in an address space do not convert: there the cast is a plain one.)
#if defined(__HIP_DEVICE_COMPILE__)
#define GLOB(T, p) ((__attribute__((address_space(1))) T*)(p))
#else
#define GLOB(T, p) ((T*)(p))
#endif
// A 16-B record through a global pointer: uint4 is a class type whose copy
// goes through a generic reference (a flat access again), a native vector is not
typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 loadGlobal4(const uint4* p) {
    const U32x4 v = *GLOB(const U32x4, p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

constexpr uint32_t kSeedChunk = 64;   // seeds a wave takes per atomic
// text tasks a wave takes per atomic (<= 64; 64 / 32 / 16 measured 1088 / 1021 /
// 891M reads/s at C3, profiles/r05_task_chunk_ab.txt)
constexpr uint32_t kTaskChunk = 64;
static_assert(kTaskChunk >= 1 && kTaskChunk <= 64, "a chunk's records sit one per lane");
constexpr uint32_t kHitChunk = 64;    // hit / task slots a wave reserves per atomic

// Per-wave slot reservation for append-only outputs (hits, tasks): ballot +
// prefix count inside the wave's current range; a fresh range of kHitChunk
// slots costs one atomic. All lanes must call it (wave-uniform).
struct SlotRange {
    uint32_t next = 0, end = 0;
    __device__ __forceinline__ bool take(bool want, uint32_t lane, uint64_t ltMask, uint32_t* counter,
                                         uint32_t& slot) {
        const uint64_t m = __ballot(want);
        if (!m) return false;
        const uint32_t cnt = (uint32_t)__popcll(m);
        const uint32_t rank = (uint32_t)__popcll(m & ltMask);
        const uint32_t avail = end - next;
        uint32_t base = 0;
        if (cnt > avail) {
            if (lane == 0) base = atomicAdd(counter, kHitChunk);
            base = __shfl(base, 0);
        }
        slot = rank < avail ? next + rank : base + (rank - avail);
        if (cnt > avail) { next = base + (cnt - avail); end = base + kHitChunk; }
        else next += cnt;
        return true;
    }
    // unused tail of the last range: empty records (len 0) for the locate scan
    __device__ __forceinline__ void close(uint32_t lane, uint4* buf, uint32_t cap) {
        for (uint32_t i = next + lane; i < end; i += 64)
            if (i < cap) buf[i] = make_uint4(0u, 0u, 0u, 0u);
    }
};

// Work queue split into kStripes stripes with one counter each (128 B apart):
// a wave starts on the stripe of its XCD (blockIdx % 8) and moves on when it
// is drained. A single counter serialises at ~90 chunk grabs per microsecond
// device-wide; eight of them keep a chunk grab off the critical path.
constexpr uint32_t kStripes = 8;
constexpr uint32_t kStripeStride = 32;  // u32 between counters
static_assert(kStripes * kStripeStride == kQueueWords, "a striped queue is one region of Ctx::Slot::queues");
struct StripedQueue {
    uint32_t* ctr;
    uint32_t n, stripe, tries = 0;
    __device__ StripedQueue(uint32_t* c, uint32_t total) : ctr(c), n(total), stripe(blockIdx.x % kStripes) {}
    // next chunk [b, e) of at most `chunk` items (wave-uniform); false when all stripes are drained
    __device__ bool next(uint32_t lane, uint32_t chunk, uint32_t& b, uint32_t& e) {
        while (tries < kStripes) {
            const uint32_t s0 = (uint32_t)((uint64_t)n * stripe / kStripes);
            const uint32_t s1 = (uint32_t)((uint64_t)n * (stripe + 1) / kStripes);
            uint32_t off = 0;
            if (lane == 0) off = s0 < s1 ? atomicAdd(ctr + stripe * kStripeStride, chunk) : 0xFFFFFFFFu;
            off = __shfl(off, 0);
            if (off != 0xFFFFFFFFu && off < s1 - s0) {
                b = s0 + off;
                e = min(b + chunk, s1);
                return true;
            }
            stripe = (stripe + 1) % kStripes;
            ++tries;
        }
        return false;
    }
};

// ---- work stealing inside a wave (wave-uniform call): of the idle lanes
// (`thief`) and the lanes that can spare their bottom stack entry (`canGive`),
// the first n = min(thieves, donors) of each pair up by rank, once stealAt
// lanes are idle. A thief (takes) reads its donor's entry and state, all lanes
// then fence (StealPlan::settle), and the donors (gives) drop the entry.
struct StealPlan {
    bool any, takes, gives;
    uint32_t donor;  // the lane a thief takes from (its own lane when !takes: shuffles by donor stay defined)
    // the thieves' reads complete before a donor's later writes reuse the entry
    __device__ __forceinline__ void settle() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};
__device__ __forceinline__ StealPlan stealPlan(bool thief, bool canGive, uint32_t stealAt, uint32_t lane,
                                               uint64_t ltMask) {
    const uint64_t I = __ballot(thief);
    const uint64_t D = __ballot(canGive);
    const uint32_t nI = (uint32_t)__popcll(I), nD = (uint32_t)__popcll(D);
    if (nI < stealAt || !nD) return {false, false, false, lane};  // wave-uniform
    const uint32_t n = min(nI, nD);
    const uint32_t r = (uint32_t)__popcll(I & ltMask);
    // donor of thief rank r: the r-th set bit of D
    uint32_t donor = 0, rr = r;
    uint64_t dm = D;
#pragma unroll
    for (uint32_t w = 32; w; w >>= 1) {
        const uint32_t c = (uint32_t)__popcll(dm & ((1ull << w) - 1ull));
        if (rr >= c) { rr -= c; dm >>= w; donor += w; }
    }
    const bool takes = thief && r < n;
    const bool gives = ((D >> lane) & 1ull) && (uint32_t)__popcll(D & ltMask) < n;
    return {true, takes, gives, takes ? donor : lane};
}

// ---- a sorted key (text position << 4 | e) of query qid -> the hit: the
// record of the position by binary search over the record starts. `starts` is
// whatever indexes to them — a global pointer or the LDS array itself, so that
// LDS reads stay ds_ reads (a pointer that may be either is generic: see the
// top). Texts of <= kLdsStarts records have their starts staged in LDS.
constexpr uint32_t kLdsStarts = 256;
template <typename Starts>
__device__ __forceinline__ sahara_hit decodeKey(uint64_t k, uint64_t qid, const Starts& starts, uint32_t nrec) {
    const uint64_t gpos = k >> 4;
    uint32_t lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= gpos) lo = mid; else hi = mid;
    }
    sahara_hit h;
    h.qid = qid;
    h.seq_id = lo;
    h.err = (uint32_t)(k & 15u);
    h.pos = gpos - starts[lo];
    return h;
}

// ---- the canonical order of hit records (the comparator of the rocPRIM
// sorts and merges that work on whole hits)
struct HitLess {
    __host__ __device__ bool operator()(const sahara_hit& a, const sahara_hit& b) const {
        if (a.qid != b.qid) return a.qid < b.qid;
        if (a.seq_id != b.seq_id) return a.seq_id < b.seq_id;
        if (a.pos != b.pos) return a.pos < b.pos;
        return a.err < b.err;
    }
};

}  // namespace
}  // namespace sahara
