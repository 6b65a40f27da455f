// search.hip — search-scheme DFS + locate on the GPU-resident FM-index (gfx950).
//
// Replaces fmc::search_ng24::search<Edit> (/root/reference/src/sahara/search.cpp:227,230)
// and fmc::LocateLinear (search.cpp:244-250) — semantics policy P0,
// docs/semantics.md; CPU restatement in oracle/oracle.cpp (Searcher::visit).
//
// Two phases per batch of patterns, both "one lane = one depth-first search,
// the wave shares a work queue":
//
// Phase 1, kSearchFM: work items are (pattern, search) pairs. Each node ranks
// all sigma-1 symbols at lo and lo+len on the BWT of its extension side — one
// 64-B Occ line per distinct 64-row block. Lanes of a pair fetch each other's
// lines together (<= 32 distinct lines per load instruction: address
// translation stays off the critical path on a multi-GB index, see
// tools/gather_bench.hip) and swap halves with DPP. As soon as a node's
// interval holds at most `split` rows, the node is handed to phase 2 as one
// *text task* per row instead of being ranked further.
//
// Phase 2, kSearchTextBatch (search_text.hip): a text task is a node whose
// string t has a single occurrence. Extending it by symbol c is non-empty iff
// c is the text's own next symbol, so the rest of its subtree is the same DFS
// run against the text. The lane copies the window of the text that the
// subtree can reach (full SA: one read) and the pattern, both as 3-bit-plane
// blocks, into LDS and expands the subtree there, without touching HBM
// (text_step.h: the step). Nodes whose remaining positions admit no further
// error are decided 32 symbols per comparison of the pattern against the window.
//
// Both DFSs push the match child first and the error children above it and
// continue with one error child in registers, so a stack holds at most the
// siblings of the error edges on the current path: <= k*(2*sigma-2) (FM) or
// <= 2k (text) entries, independent of the pattern length.
//
// The multiset of (qid, text position, e) leaves equals the reference DFS's:
// a node of interval [lb, lb+len) expands to the same (path, occurrence)
// pairs whether it is ranked or split into its len occurrences.
//
// Leaves are compacted into the hit buffer with a wave ballot + prefix count
// into per-wave reserved slot ranges (one atomic per 64 slots). Overflow of
// any buffer is flagged; the host re-runs the batch with a larger buffer.
//
// Locate: FM leaves resolve rows through the resident full SA (one read per
// row) or, in the reference mode, by LF walks to the SA samples, straight
// into per-query segments (counting sort by qid: row counts, exclusive scan).
// Keys text position << 4 | e are then sorted within each segment — in
// registers for the usual <= 8 rows, by a segmented radix sort for longer
// segments — for the canonical (qid, seq_id, pos, e) order.

#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "search_device.h"

namespace sahara {
namespace {

// Swap a dword with the neighbour lane of the pair (DPP quad_perm [1,0,3,2]).
__device__ __forceinline__ uint32_t pairSwap(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ uint4 pairSwap4(const uint4& v) {
    return make_uint4(pairSwap(v.x), pairSwap(v.y), pairSwap(v.z), pairSwap(v.w));
}
__device__ __forceinline__ uint64_t pairSwap64(uint64_t v) {
    return (uint64_t)pairSwap((uint32_t)v) | ((uint64_t)pairSwap((uint32_t)(v >> 32)) << 32);
}

// Pair-cooperative fetch of the rank part (bytes 0..47) of one 64-B Occ line
// per lane. Must be called by all 64 lanes (wave-uniform control flow):
// for the pair (E = even lane's line, O = odd lane's line) four loads run
//   #1 E bytes 0-15 | 16-31   #2 E bytes 32-47 | 48-63
//   #3 O bytes 0-15 | 16-31   #4 O bytes 32-47 | 48-63
// (even | odd lane), so each wave instruction touches <= 32 distinct lines;
// two DPP swaps then hand each lane the chunks of its own line.
__device__ __forceinline__ void fetchLinePair(uint64_t own, bool need, bool odd, uint32_t cnt[5], uint64_t p[3]) {
    const uint64_t other = pairSwap64(own);
    const bool otherNeed = pairSwap(need ? 1u : 0u) != 0u;
    const uint64_t addrE = odd ? other : own, addrO = odd ? own : other;
    const bool needE = odd ? otherNeed : need, needO = odd ? need : otherNeed;
    const uint32_t half = odd ? 16u : 0u;
    uint4 r1 = make_uint4(0, 0, 0, 0), r2 = r1, r3 = r1, r4 = r1;
    if (needE) {
        r1 = loadGlobal4(reinterpret_cast<const uint4*>(addrE + half));
        r2 = loadGlobal4(reinterpret_cast<const uint4*>(addrE + 32 + half));
    }
    if (needO) {
        r3 = loadGlobal4(reinterpret_cast<const uint4*>(addrO + half));
        r4 = loadGlobal4(reinterpret_cast<const uint4*>(addrO + 32 + half));
    }
    // even: r1 = E0, r2 = E2, r3 = O0, r4 = O2 ; odd: r1 = E1, r2 = E3, r3 = O1, r4 = O3
    const uint4 g1 = pairSwap4(odd ? r1 : r3);  // even <- E1, odd <- O0
    const uint4 g2 = pairSwap4(r4);             // odd <- O2 (even receives O3, unused)
    const uint4 c0 = odd ? g1 : r1;
    const uint4 c1 = odd ? r3 : g1;
    const uint4 c2 = odd ? g2 : r2;
    cnt[0] = c0.x; cnt[1] = c0.y; cnt[2] = c0.z; cnt[3] = c0.w; cnt[4] = c1.x;
    p[0] = (uint64_t)c1.z | ((uint64_t)c1.w << 32);
    p[1] = (uint64_t)c2.x | ((uint64_t)c2.y << 32);
    p[2] = (uint64_t)c2.z | ((uint64_t)c2.w << 32);
}

__device__ __forceinline__ uint32_t pick5(const uint32_t v[5], uint32_t i) {
    uint32_t r = v[0];
    r = i == 1 ? v[1] : r;
    r = i == 2 ? v[2] : r;
    r = i == 3 ? v[3] : r;
    r = i == 4 ? v[4] : r;
    return r;
}

__device__ __forceinline__ uint32_t nib(uint32_t word, uint32_t i) { return (word >> ((i & 7u) * 4u)) & 0xFu; }

// Children of one DFS node under policy P0 (docs/semantics.md), with the
// stack discipline described at the top. `occ[c]` says whether the child of
// symbol c exists; `mk(c, kind)` builds it. Returns whether a child is kept
// in registers (through `next`).
template <int SIGMA, typename Node, typename MkChild, typename Push>
__device__ __forceinline__ bool expandChildren(const uint32_t occ[SIGMA], uint32_t cq, bool matchOK, bool misOK,
                                               bool delOK, bool insOK, const Node& insChild, MkChild mk, Push push,
                                               Node& next) {
    uint32_t nErr = insOK ? 1u : 0u;
    bool hasM = false;
#pragma unroll
    for (int c = 1; c < SIGMA; ++c) {
        if (occ[c]) {
            if ((uint32_t)c == cq) hasM = matchOK;
            else nErr += misOK ? 1u : 0u;
            nErr += delOK ? 1u : 0u;
        }
    }
    bool kept = false;
    auto emit = [&](const Node& v) {
        if (!kept) { next = v; kept = true; }
        else push(v);
    };
    if (hasM && nErr) push(mk((int)cq, 0));  // match child below all its error siblings
    if (insOK) emit(insChild);
#pragma unroll
    for (int c = 1; c < SIGMA; ++c) {
        if (occ[c]) {
            if ((uint32_t)c != cq && misOK) emit(mk(c, 1));
            if (delOK) emit(mk(c, 2));
        }
    }
    if (!kept && hasM) { next = mk((int)cq, 0); kept = true; }
    return kept;
}

// kind: 0 = match (M), 1 = substitution (S), 2 = deletion (D), 3 = insertion (I)
__device__ __forceinline__ uint32_t childMeta(uint32_t pos, uint32_t e, uint32_t lastL, uint32_t lastR, bool right,
                                              uint32_t dl, uint32_t kind) {
    const uint32_t op = kind == 2 ? OP_D : (kind == 3 ? OP_I : OP_MS);
    const uint32_t npos = kind == 2 ? pos : pos + 1u;
    const uint32_t ne = kind == 0 ? e : e + 1u;
    const uint32_t nl = pos == 0 ? op : (right ? lastL : op);
    const uint32_t nr = pos == 0 ? op : (right ? op : lastR);
    const uint32_t nd = dl + (kind == 2 ? 1u : 0u) - (kind == 3 ? 1u : 0u);
    return npos | (ne << 16) | (nl << 20) | (nr << 22) | (nd << 25);
}

// ========================================================= seeds ====
// One thread per work item (pattern, search): its starting cursor. A search
// whose first kmerK steps admit no error starts at depth kmerK from the k-mer
// table (the DFS would reach the same node through kmerK forced matches);
// items whose k-mer does not occur end here. Every other item starts at the
// root. Surviving items are appended (wave ballot + one atomic per wave) to
// the seed list that kSearchFM consumes.
// The k-mer table index of item i's error-free first part, or ~0u when the
// item starts at the root (no table, no error-free first part, or an N in it).
template <int SIGMA>
__device__ __forceinline__ uint32_t seedCode(const SeedArgs& a, uint32_t i) {
    if (i >= a.nitems || !a.kmer) return ~0u;
    const uint32_t pid = i / a.nsearch, s = i - pid * a.nsearch;
    const uint32_t ks = a.kmerStart[s];
    if (ks == 0xFFFFFFFFu) return ~0u;
    const uint32_t* pw = a.pats + (size_t)pid * a.patWords + (ks >> 3);
    const uint32_t w0 = pw[0], w1 = pw[1], w2 = pw[2];
    const uint32_t sh = (ks & 7u) * 4u;
    const uint64_t run = (uint64_t)__builtin_amdgcn_alignbit(w1, w0, sh) |
                         ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, sh) << 32);
    uint32_t code = 0;
    bool acgt = true;
    for (uint32_t j = 0; j < a.kmerK; ++j) {
        const uint32_t c = (uint32_t)(run >> (4u * j)) & 0xFu;  // A1 C2 G3 (N4) T5|T4
        acgt = acgt && !(SIGMA == 6 && c == 4u);
        code = code * 4u + ((SIGMA == 6 && c == 5u) ? 3u : c - 1u);
    }
    return acgt ? (uint32_t)(code & ((1ull << (2u * a.kmerK)) - 1ull)) : ~0u;
}

// Item i's starting cursor: the k-mer table entry of its error-free first
// part (depth kmerK), else the root. The two lanes of a pair fetch each
// other's 16-B entries cooperatively — each lane 8 B of the even lane's entry,
// then 8 B of the odd lane's, swapped back with DPP — so that a load
// instruction touches at most 32 distinct lines of the 68.7 GB table (address
// translation, not bandwidth, bounds these random lookups: tools/gather_bench).
// Must be called by all lanes of the wave.
template <int SIGMA>
__device__ __forceinline__ uint4 seedOf(const SeedArgs& a, uint32_t i, bool& keep, uint32_t& textPos,
                                        bool& skipped) {
    keep = i < a.nitems;
    // besthits: the pattern reported in an earlier round (nothing writes the
    // counts while the seeds run: pass.cpp issueFM)
    skipped = keep && a.skip && a.skip[i / a.nsearch] != 0u;
    keep = keep && !skipped;
    const uint32_t code = keep ? seedCode<SIGMA>(a, i) : ~0u;
    const bool need = keep && code != ~0u;
    const bool odd = (threadIdx.x & 1u) != 0u;
    const uint64_t own = (uint64_t)(a.kmer + (need ? code : 0u));
    const uint64_t other = pairSwap64(own);
    const bool otherNeed = pairSwap(need ? 1u : 0u) != 0u;
    const uint64_t addrE = odd ? other : own, addrO = odd ? own : other;
    const bool needE = odd ? otherNeed : need, needO = odd ? need : otherNeed;
    const uint32_t half = odd ? 8u : 0u;
    uint2 rE = make_uint2(0u, 0u), rO = rE;
    if (needE) rE = *reinterpret_cast<const uint2*>(addrE + half);  // even's entry: bytes 0-7 | 8-15
    if (needO) rO = *reinterpret_cast<const uint2*>(addrO + half);  // odd's entry: bytes 0-7 | 8-15
    const uint2 gE = make_uint2(pairSwap(rE.x), pairSwap(rE.y));     // even <- bytes 8-15 of its entry
    const uint2 gO = make_uint2(pairSwap(rO.x), pairSwap(rO.y));     // odd <- bytes 0-7 of its entry
    const uint4 t = odd ? make_uint4(gO.x, gO.y, rO.x, rO.y) : make_uint4(rE.x, rE.y, gE.x, gE.y);
    textPos = t.w;  // SA[lb] when the k-mer occurs once (DeviceIndex::kmerPos)
    if (!need) return make_uint4(0u, 0u, a.n, kDeltaZero);
    keep = t.z != 0u;
    return make_uint4(t.x, t.y, t.z, packMeta(a.kmerK, 0u, OP_MS, OP_MS));
}

// Each block takes 1024 consecutive items per round (4 per thread, so four
// table lookups are in flight per lane) and appends the survivors with one
// atomic per round and output list: seeds for the FM kernel, and text tasks
// for seeds whose k-mer occurs exactly once (toText) — the node the FM kernel
// would hand to the text phase at once.
template <int SIGMA>
__global__ __launch_bounds__(256) void kSeedItems(SeedArgs a) {
    __shared__ uint32_t wcount[2][4], blockBase[2];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t ltMask = (1ull << lane) - 1ull;
    uint64_t cTasks = 0, cSkipped = 0;
    for (uint32_t base = a.itemBegin + blockIdx.x * 1024u; base < a.nitems; base += gridDim.x * 1024u) {  // block-uniform
        uint4 cur[4];
        uint32_t tpos[4];
        bool keep[4], task[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool skipped;
            cur[k] = seedOf<SIGMA>(a, base + k * 256u + threadIdx.x, keep[k], tpos[k], skipped);
            cSkipped += skipped ? 1u : 0u;
            task[k] = keep[k] && a.toText && cur[k].z == 1u && (cur[k].w & 0xFFFFu) < a.m;
            keep[k] = keep[k] && !task[k];
        }
        uint64_t m[4], mt[4];
        uint32_t wsum = 0, wtask = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = __ballot(keep[k]);
            mt[k] = __ballot(task[k]);
            wsum += (uint32_t)__popcll(m[k]);
            wtask += (uint32_t)__popcll(mt[k]);
        }
        if (lane == 0) { wcount[0][w] = wsum; wcount[1][w] = wtask; }
        __syncthreads();
        if (threadIdx.x < 2) {
            const uint32_t* wc = wcount[threadIdx.x];
            const uint32_t tot = wc[0] + wc[1] + wc[2] + wc[3];
            blockBase[threadIdx.x] = tot ? atomicAdd(threadIdx.x ? a.taskCount : a.seedCount, tot) : 0u;
        }
        __syncthreads();
        uint32_t slot = blockBase[0], tslot = blockBase[1];
        for (uint32_t j = 0; j < w; ++j) { slot += wcount[0][j]; tslot += wcount[1][j]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t item = base + k * 256u + threadIdx.x;
            if (keep[k]) {
                const uint32_t at = slot + (uint32_t)__popcll(m[k] & ltMask);
                a.seeds[at] = cur[k];
                a.seedItem[at] = item;
            }
            if (task[k]) {  // (row, |t| = kmerK, pattern, node meta | search << 24), or with
                            // the text position instead of the row (kTaskPos)
                const uint32_t at = tslot + (uint32_t)__popcll(mt[k] & ltMask);
                const uint32_t pid = item / a.nsearch, sIdx = item - pid * a.nsearch;
                if (at < a.taskCap)
                    a.tasks[at] = make_uint4(a.kmerPos ? tpos[k] : cur[k].x,
                                             (cur[k].w & 0xFFFFu) | (a.kmerPos ? kTaskPos : 0u), pid,
                                             (cur[k].w & 0x00FFFFFFu) | (sIdx << 24));
                else
                    atomicOr(a.flags, kFlagTasks);
                ++cTasks;
            }
            slot += (uint32_t)__popcll(m[k]);
            tslot += (uint32_t)__popcll(mt[k]);
        }
        __syncthreads();  // wcount / blockBase reused next round
    }
    if (a.counters && cTasks) {
        atomicAdd(a.counters + kCtTextTasks, (unsigned long long)cTasks);
        if (a.kmerPos) atomicAdd(a.counters + kCtPosTasks, (unsigned long long)cTasks);
    }
    if (a.counters && cSkipped) atomicAdd(a.counters + kCtBestSkipped, (unsigned long long)cSkipped);
}

// =========================================================== phase 1: FM ====

template <int SIGMA, bool EDIT, bool COUNT>
__global__ __launch_bounds__(256) void kSearchFM(SearchArgs a) {
    extern __shared__ uint32_t sch[];
    for (uint32_t i = threadIdx.x; i < a.nsearch * a.m; i += blockDim.x) sch[i] = a.scheme[i];
    __syncthreads();

    const uint32_t T = gridDim.x * blockDim.x;
    const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ltMask = (1ull << lane) - 1ull;
    const bool odd = lane & 1u;
    // DFS stack: the bottom a.ldsDepth levels live in LDS after the scheme
    // table ([level][thread], conflict-free 16-B rows when lanes sit at equal
    // depth), deeper levels spill to HBM ([level][grid thread]).
    uint4* lstk = reinterpret_cast<uint4*>(sch + ((a.nsearch * a.m + 3u) & ~3u));
    const uint32_t ldsDepth = a.ldsDepth;
    uint4* stk = a.stack + gtid;

    // the lane's stack holds entries [bot, sp) in a ring of stackLevels levels
    // (entry d at level d mod stackLevels; bot < stackLevels): pushes and pops
    // at sp, work stealing takes the bottom entry (bot++)
    uint32_t sp = 0, bot = 0, pid = 0, sIdx = 0;
    bool have = false, exhausted = false;
    uint32_t qNext = 0, qEnd = 0, filled = 0;  // wave-uniform
    bool qDone = false;
    SlotRange hitSlots, taskSlots;
    uint4 cur = make_uint4(0, 0, 0, 0);
    uint64_t cNodes = 0, cRank = 0, cLines = 0, cTasks = 0, cIter = 0;
    const uint32_t L = a.stackLevels;
    auto stackGet = [&](uint32_t d) -> uint4 {
        d = d >= L ? d - L : d;
        return d < ldsDepth ? lstk[d * 256u + threadIdx.x] : stk[(size_t)(d - ldsDepth) * T];
    };
    auto stackPut = [&](uint32_t d, const uint4& v) {
        d = d >= L ? d - L : d;
        if (d < ldsDepth) lstk[d * 256u + threadIdx.x] = v;
        else stk[(size_t)(d - ldsDepth) * T] = v;
    };
    // seeds (kSeedItems: starting cursor + item) arrive in chunks of 64, one
    // record per lane, prefetched a chunk ahead so a refill costs no memory trip
    const uint32_t nseeds = *a.seedCount;
    uint4 curRec = make_uint4(0, 0, 0, 0), nextRec = curRec;
    uint32_t curItem = 0, nextItem = 0, nBase = 0, nEnd = 0, qBase = 0;
    bool haveNext = false;
    StripedQueue queue(a.work, nseeds);
    {
        uint32_t b = 0, e = 0;
        if (queue.next(lane, kSeedChunk, b, e)) {
            nBase = b;
            nEnd = e;
            if (b + lane < e) { nextRec = a.seeds[b + lane]; nextItem = a.seedItem[b + lane]; }
            haveNext = true;
        } else {
            qDone = true;
        }
    }

    for (;;) {
        // ---- refill idle lanes from the wave's current seed chunk
        const bool need = !have && sp == bot && !exhausted;
        uint64_t pending = __ballot(need);
        while (pending) {  // wave-uniform
            if (qNext >= qEnd) {
                if (!haveNext) break;
                qBase = nBase;
                qNext = nBase;
                qEnd = nEnd;
                curRec = nextRec;
                curItem = nextItem;
                haveNext = false;
                if (!qDone) {
                    uint32_t b = 0, e = 0;
                    if (!queue.next(lane, kSeedChunk, b, e)) {
                        qDone = true;
                    } else {
                        nBase = b;
                        nEnd = e;
                        if (b + lane < e) { nextRec = a.seeds[b + lane]; nextItem = a.seedItem[b + lane]; }
                        haveNext = true;
                    }
                }
                if (qNext >= qEnd) continue;
            }
            const uint32_t take = min(qEnd - qNext, (uint32_t)__popcll(pending));
            const uint32_t rank = (uint32_t)__popcll(pending & ltMask);
            const bool mine = ((pending >> lane) & 1ull) && rank < take;
            const uint32_t src = (qNext - qBase + rank) & 63u;
            const uint4 sd = make_uint4(__shfl(curRec.x, src), __shfl(curRec.y, src), __shfl(curRec.z, src),
                                        __shfl(curRec.w, src));
            const uint32_t item = __shfl(curItem, src);
            if (mine) {
                pid = item / a.nsearch;
                sIdx = item - pid * a.nsearch;
                cur = sd;
                have = true;
            }
            pending &= ~__ballot(mine);
            qNext += take;
        }
        if (qDone && !haveNext && qNext >= qEnd && need && !have) exhausted = true;
        if (!have && sp > bot) {
            --sp;
            cur = stackGet(sp);
            have = true;
        }
        if (sp == bot) sp = bot = 0;
        // ---- work stealing inside the wave once the seed queue is dry (wave-
        // uniform: the queue state is the wave's). The DFS of one seed varies
        // by orders of magnitude in size (repeats, and from the root every
        // search ranks thousands of nodes at k = 3), so a launch otherwise ends
        // with most lanes idle beside a few long ones (reference execution at
        // C5: lanes busy 0.49). An idle lane takes the bottom (shallowest, so
        // largest) stack entry of the r-th busy lane, with its pattern id and
        // search by shuffle; the entry's subtree is the same DFS whichever lane
        // runs it, so the leaves are too.
        if (a.stealAt && qDone && !haveNext && qNext >= qEnd) {
            const bool thief = !have;
            const uint64_t I = __ballot(thief);
            const uint64_t D = __ballot(have && sp > bot);
            const uint32_t nI = (uint32_t)__popcll(I), nD = (uint32_t)__popcll(D);
            if (nI >= a.stealAt && nD) {  // wave-uniform
                const uint32_t n = min(nI, nD);
                const uint32_t r = (uint32_t)__popcll(I & ltMask);
                uint32_t donor = 0, rr = r;
                uint64_t dm = D;
#pragma unroll
                for (uint32_t w = 32; w; w >>= 1) {  // the r-th set bit of D
                    const uint32_t c = (uint32_t)__popcll(dm & ((1ull << w) - 1ull));
                    if (rr >= c) { rr -= c; dm >>= w; donor += w; }
                }
                const bool takes = thief && r < n;
                donor = takes ? donor : lane;
                const uint32_t dPid = __shfl(pid, donor), dS = __shfl(sIdx, donor), dBot = __shfl(bot, donor);
                if (takes) {
                    const uint32_t dt = (threadIdx.x & ~63u) | donor;
                    const uint32_t lv = dBot;  // < L
                    if (lv < ldsDepth) cur = lstk[lv * 256u + dt];
                    else cur = loadGlobal4(a.stack + (size_t)(lv - ldsDepth) * T + (gtid & ~63u) + donor);
                    pid = dPid;
                    sIdx = dS;
                    have = true;
                }
                // the thieves' reads complete before a donor's later pushes
                // can reuse the level (its stack emptied and reset)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (((D >> lane) & 1ull) && (uint32_t)__popcll(D & ltMask) < n && ++bot == L) {
                    bot = 0;
                    sp -= L;
                }
            }
        }
        if (!__any(have)) break;
        if (COUNT && lane == 0) ++cIter;

        const uint32_t pos = cur.w & 0xFFFFu;
        // ---- leaves -> hit buffer
        {
            const bool leaf = have && pos == a.m;
            uint32_t slot;
            if (hitSlots.take(leaf, lane, ltMask, a.hitCount, slot) && leaf) {
                if (slot < a.hitCap) {
                    a.hits[slot] = make_uint4(pid, cur.x, cur.z, (cur.w >> 16) & 0xFu);
                    a.rank[slot] = atomicAdd(a.qcnt + pid, cur.z);  // its first row's place in the query's segment
                } else {
                    atomicOr(a.flags, kFlagHits);
                }
                have = false;
                ++filled;
            }
        }
        // ---- small intervals -> one text task per row (phase 2)
        if (a.split) {
            const bool conv = have && cur.z <= a.split;
            const uint32_t tlen = pos + metaDelta(cur.w) - 16u;  // |t|
            for (uint32_t j = 0; __any(conv && j < cur.z); ++j) {  // wave-uniform trip count
                const bool want = conv && j < cur.z;
                uint32_t slot;
                if (taskSlots.take(want, lane, ltMask, a.taskCount, slot) && want) {
                    if (slot < a.taskCap)
                        a.tasks[slot] = make_uint4(cur.x + j, tlen, pid, (cur.w & 0x00FFFFFFu) | (sIdx << 24));
                    else atomicOr(a.flags, kFlagTasks);
                    if (COUNT) ++cTasks;
                }
            }
            if (conv) have = false;
        }

        // ---- decode the node (per lane)
        uint32_t e = 0, lastL = 0, lastR = 0, cq = 0;
        bool right = false, matchOK = false, misOK = false, delOK = false, insOK = false;
        uint32_t lo = 0, hi = 0;
        bool needA = false, needB = false;
        if (have) {
            e = (cur.w >> 16) & 0xFu;
            lastL = (cur.w >> 20) & 3u;
            lastR = (cur.w >> 22) & 3u;
            const uint32_t se = sch[sIdx * a.m + pos];
            const uint32_t q = se & 0xFFFFu, lb = (se >> 16) & 0xFu, ub = (se >> 20) & 0xFu;
            right = (se >> 24) & 1u;
            cq = nib(a.pats[(size_t)pid * a.patWords + (q >> 3)], q);
            const uint32_t side = right ? lastR : lastL;
            matchOK = lb <= e && e <= ub;
            misOK = lb <= e + 1 && e + 1 <= ub;
            delOK = EDIT && pos > 0 && e + 1 <= ub && side != OP_I;
            insOK = EDIT && misOK && side != OP_D;
            lo = right ? cur.y : cur.x;
            hi = lo + cur.z;
            needA = matchOK || misOK || delOK;
            needB = needA && (hi >> 6) != (lo >> 6);
        }

        // ---- pair-cooperative Occ line fetch (wave-uniform)
        const uint64_t ownA = (uint64_t)(right ? a.occR : a.occF) + (uint64_t)(lo >> 6) * 64u;
        const uint64_t ownB = (uint64_t)(right ? a.occR : a.occF) + (uint64_t)(hi >> 6) * 64u;
        uint32_t ca[5], cb[5];
        uint64_t pa[3], pb[3];
        fetchLinePair(ownA, needA, odd, ca, pa);
        fetchLinePair(ownB, needB, odd, cb, pb);

        if (have) {
            if (COUNT) ++cNodes;
            // child c = (fx[c], fy[c], occ[c]): forward / reverse lower bounds
            uint32_t occ[SIGMA], fx[SIGMA], fy[SIGMA];
#pragma unroll
            for (int c = 0; c < SIGMA; ++c) occ[c] = fx[c] = fy[c] = 0;
            if (needA) {
                if (!needB) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) cb[i] = ca[i];
                    pb[0] = pa[0]; pb[1] = pa[1]; pb[2] = pa[2];
                }
                if (COUNT) { ++cRank; cLines += needB ? 2 : 1; }
                const uint64_t ml = lowMask(lo & 63u), mh = lowMask(hi & 63u);
                uint32_t sum = 0, base[SIGMA];
#pragma unroll
                for (int c = 1; c < SIGMA; ++c) {
                    const uint32_t rl = ca[c - 1] + (uint32_t)__popcll(symMask(pa, c) & ml);
                    const uint32_t rh = cb[c - 1] + (uint32_t)__popcll(symMask(pb, c) & mh);
                    occ[c] = rh - rl;
                    base[c] = a.C[c] + rl;
                    sum += occ[c];
                }
                // bidirectional update: the other side moves by the occurrences
                // of the smaller symbols, '$' first
                uint32_t acc = (right ? cur.x : cur.y) + (cur.z - sum);
#pragma unroll
                for (int c = 1; c < SIGMA; ++c) {
                    fx[c] = right ? acc : base[c];
                    fy[c] = right ? base[c] : acc;
                    acc += occ[c];
                }
            }
            const uint32_t dl = metaDelta(cur.w);
            auto mk = [&](int c, uint32_t kind) -> uint4 {
                uint32_t f = 0, g = 0, o = 0;
#pragma unroll
                for (int s = 1; s < SIGMA; ++s)
                    if (s == c) { f = fx[s]; g = fy[s]; o = occ[s]; }
                return make_uint4(f, g, o, childMeta(pos, e, lastL, lastR, right, dl, kind));
            };
            auto push = [&](const uint4& v) {
                if (sp - bot < a.stackCap) {
                    stackPut(sp, v);
                    ++sp;
                } else {
                    atomicOr(a.flags, kFlagStack);
                }
            };
            const uint4 ins = make_uint4(cur.x, cur.y, cur.z, childMeta(pos, e, lastL, lastR, right, dl, 3));
            uint4 next = make_uint4(0, 0, 0, 0);
            have = expandChildren<SIGMA>(occ, cq, matchOK, misOK, delOK, insOK, ins, mk, push, next);
            cur = next;
        }
    }
    hitSlots.close(lane, a.hits, a.hitCap);
    taskSlots.close(lane, a.tasks, a.taskCap);
    if (filled) atomicAdd(a.filled, filled);  // per-lane counts
    if (COUNT) {
        atomicAdd(a.counters + kCtNodes, (unsigned long long)cNodes);
        atomicAdd(a.counters + kCtRankNodes, (unsigned long long)cRank);
        atomicAdd(a.counters + kCtExtLines, (unsigned long long)cLines);
        atomicAdd(a.counters + kCtTextTasks, (unsigned long long)cTasks);
        if (cIter) atomicAdd(a.counters + kCtFmIter, (unsigned long long)cIter);
    }
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

__device__ __forceinline__ sahara_hit decodeKey(uint64_t k, uint64_t qid, const uint64_t* __restrict__ starts,
                                                uint32_t nrec) {
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

__device__ __forceinline__ void cswap(uint64_t& a, uint64_t& b) {
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Sort + decode, one workgroup per 256 consecutive queries. Their segments
// are one contiguous key range; when it fits kTileKeys (the common case: ~1.3
// rows per query) it is staged in LDS by coalesced loads, every segment is
// sorted there, and the decoded hits leave as one coalesced run of 24-B
// records. Per segment: <= kSmallSeg rows sorted in the lane's registers
// (odd-even transposition, padded with ~0); medium ones by the wave, one key
// per lane, bitonic over shuffles; long ones are left to the segmented radix
// sort (kDecodeBig). Record starts sit in LDS for texts of <= kLdsStarts
// records, so a decode's binary search waits on no global loads. A range
// larger than the tile takes the same tiers straight from global memory.
constexpr uint32_t kTileKeys = 1024;
constexpr uint32_t kLdsStarts = 256;
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
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const bool ldsStarts = !COMPACT && nrec <= kLdsStarts;
    if (ldsStarts)
        for (uint32_t i = t; i < nrec; i += 256) sst[i] = starts[i];
    auto decode = [&](uint64_t k, uint64_t qid) {
        const uint64_t gpos = k >> 4;
        uint32_t lo = 0, hi = nrec;
        uint64_t s0 = 0;
        if (ldsStarts) {
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sst[mid] <= gpos) lo = mid; else hi = mid;
            }
            s0 = sst[lo];
        } else {
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (starts[mid] <= gpos) lo = mid; else hi = mid;
            }
            s0 = starts[lo];
        }
        sahara_hit h;
        h.qid = qid;
        h.seq_id = lo;
        h.err = (uint32_t)(k & 15u);
        h.pos = gpos - s0;
        return h;
    };
    // sorted key k of the batch's query lq -> out[i]
    auto put = [&](uint64_t i, uint64_t k, uint32_t lq) {
        if constexpr (COMPACT) out[i] = compactRecord(k, lq);
        else out[i] = decode(k, qidBase + lq);
    };
    for (uint32_t q0 = blockIdx.x * 256u; q0 < nq; q0 += gridDim.x * 256u) {
        const uint32_t q = q0 + t;
        soff[t] = qoff[q < nq ? q : nq];
        if (t == 0) soff[256] = qoff[q0 + 256u < nq ? q0 + 256u : nq];
        __syncthreads();
        const uint64_t base = soff[0], R = soff[256] - base;
        const uint64_t b = soff[t];
        const uint32_t n = q < nq ? (uint32_t)(soff[t + 1] - b) : 0u;
        if (R <= kTileKeys) {  // block-uniform
            for (uint32_t i = t; i < (uint32_t)R; i += 256) sk[i] = keys[base + i];
            __syncthreads();
            const uint32_t lb = (uint32_t)(b - base);
            if (n && n <= kSmallSeg) {
                uint64_t v[kSmallSeg];
#pragma unroll
                for (uint32_t i = 0; i < kSmallSeg; ++i) v[i] = i < n ? sk[lb + i] : ~0ull;
#pragma unroll
                for (uint32_t r = 0; r < kSmallSeg; ++r) {
                    if (r >= n) break;
#pragma unroll
                    for (uint32_t i = r & 1u; i + 1 < kSmallSeg; i += 2) cswap(v[i], v[i + 1]);
                }
#pragma unroll
                for (uint32_t i = 0; i < kSmallSeg; ++i)
                    if (i < n) {
                        sk[lb + i] = v[i];
                        sq[lb + i] = (uint16_t)t;
                    }
            } else if (n > kMediumSeg) {
                for (uint32_t i = 0; i < n; ++i) sq[lb + i] = kSkipRow;  // the radix path decodes it
            }
            uint64_t med = __ballot(n > kSmallSeg && n <= kMediumSeg);
            while (med) {
                const int src = __ffsll((long long)med) - 1;
                med &= med - 1;
                const uint32_t sn = (uint32_t)__shfl((int)n, src), slb = (uint32_t)__shfl((int)lb, src);
                uint64_t v = lane < sn ? sk[slb + lane] : ~0ull;
#pragma unroll
                for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        const uint64_t o = __shfl_xor(v, j);
                        const bool keepMin = ((lane & j) == 0) == ((lane & k) == 0);
                        v = keepMin ? (v < o ? v : o) : (v < o ? o : v);
                    }
                }
                if (lane < sn) {
                    sk[slb + lane] = v;
                    sq[slb + lane] = (uint16_t)((t & ~63u) + (uint32_t)src);
                }
            }
            __syncthreads();
            for (uint32_t i = t; i < (uint32_t)R; i += 256) {
                const uint32_t lq = sq[i];
                if (lq != kSkipRow) put(base + i, sk[i], q0 + lq);
            }
            __syncthreads();  // soff, sk, sq are reused by the next range
            continue;
        }
        __syncthreads();  // soff is reused by the next range
        if (n && n <= kSmallSeg) {
            uint64_t v[kSmallSeg];
#pragma unroll
            for (uint32_t i = 0; i < kSmallSeg; ++i) v[i] = i < n ? keys[b + i] : ~0ull;
            // n rounds sort the n keys (the ~0 padding never moves)
#pragma unroll
            for (uint32_t r = 0; r < kSmallSeg; ++r) {
                if (r >= n) break;
#pragma unroll
                for (uint32_t i = r & 1u; i + 1 < kSmallSeg; i += 2) cswap(v[i], v[i + 1]);
            }
#pragma unroll
            for (uint32_t i = 0; i < kSmallSeg; ++i)
                if (i < n) put(b + i, v[i], q);
        }
        uint64_t med = __ballot(n > kSmallSeg && n <= kMediumSeg);
        while (med) {
            const int src = __ffsll((long long)med) - 1;
            med &= med - 1;
            const uint32_t sqid = (uint32_t)__shfl((int)q, src), sn = (uint32_t)__shfl((int)n, src);
            const uint64_t sb = __shfl(b, src);
            uint64_t v = lane < sn ? keys[sb + lane] : ~0ull;
#pragma unroll
            for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    const uint64_t o = __shfl_xor(v, j);
                    const bool keepMin = ((lane & j) == 0) == ((lane & k) == 0);
                    v = keepMin ? (v < o ? v : o) : (v < o ? o : v);
                }
            }
            if (lane < sn) put(sb + lane, v, sqid);
        }
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

struct SegOff {  // begin (d = 0) / end (d = 1) of a listed query's segment
    const uint64_t* qoff;
    uint32_t d;
    __host__ __device__ uint32_t operator()(const uint32_t& q) const { return (uint32_t)qoff[q + d]; }
};

// The compiled variants of kSearchFM, named once (sigma 5 or 6).
const void* searchKernel(uint32_t sigma, bool edit, bool count) {
#define SH_ROW(S, E) {(const void*)kSearchFM<S, E, false>, (const void*)kSearchFM<S, E, true>}
    static const void* const kernels[2][2][2] = {{SH_ROW(5, false), SH_ROW(5, true)}, {SH_ROW(6, false), SH_ROW(6, true)}};
#undef SH_ROW
    return kernels[sigma == 5 ? 0 : 1][edit][count];
}

}  // namespace

int searchBlocksPerCU(uint32_t sigma, bool edit, size_t lds) {
    int b = 0;
    SH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, searchKernel(sigma, edit, false), 256, lds));
    return b < 1 ? 1 : b;
}

void launchSearch(const SearchArgs& a, uint32_t sigma, bool edit, bool count, uint32_t blocks, size_t lds,
                  hipStream_t st) {
    void* args[] = {const_cast<SearchArgs*>(&a)};
    SH_HIP(hipLaunchKernel(searchKernel(sigma, edit, count), dim3(blocks), dim3(256), args, lds, st));
}


void launchSeeds(const SeedArgs& a, uint32_t sigma, uint32_t blocks, hipStream_t st) {
    if (sigma == 5) hipLaunchKernelGGL((kSeedItems<5>), dim3(blocks), dim3(256), 0, st, a);
    else            hipLaunchKernelGGL((kSeedItems<6>), dim3(blocks), dim3(256), 0, st, a);
    SH_HIP(hipGetLastError());
}

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

// Applies --max_hits n to one batch's hits (out, rows; per-query segments
// qoff[0..nq]) in place; returns the rows kept. Host-synchronous (the kept
// total sizes the rest of the batch's chain): read back through hostKept,
// 8 B of pinned memory.
uint64_t limitBatch(sahara_hit* out, uint64_t rows, const uint64_t* qoff, uint32_t nq, uint32_t n,
                    DevBuf<uint32_t>& kcnt, DevBuf<uint64_t>& koff, DevBuf<sahara_hit>& buf, DevBuf<char>& tmp,
                    uint64_t* hostKept, hipStream_t st) {
    if (rows == 0 || nq == 0) return rows;
    kcnt.reserve((size_t)nq + 1);
    koff.reserve((size_t)nq + 1);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>((nq + 256) / 256, 16384));
    hipLaunchKernelGGL(kLimitCount, dim3(blocks), dim3(256), 0, st, out, qoff, nq, n, kcnt.ptr);
    SH_HIP(hipGetLastError());
    size_t bytes = 0;
    SH_HIP(rocprim::exclusive_scan(nullptr, bytes, kcnt.ptr, koff.ptr, (uint64_t)0, (size_t)nq + 1,
                                   rocprim::plus<uint64_t>(), st));
    tmp.reserve(bytes + 256);
    SH_HIP(rocprim::exclusive_scan(tmp.ptr, bytes, kcnt.ptr, koff.ptr, (uint64_t)0, (size_t)nq + 1,
                                   rocprim::plus<uint64_t>(), st));
    SH_HIP(hipMemcpyAsync(hostKept, koff.ptr + nq, 8, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    const uint64_t kept = *hostKept;
    if (kept == rows) return rows;  // nothing to drop in this batch
    buf.reserve(std::max<uint64_t>(kept, 1));
    hipLaunchKernelGGL(kLimitWrite, dim3(blocks), dim3(256), 0, st, out, qoff, nq, n, koff.ptr, buf.ptr);
    SH_HIP(hipGetLastError());
    if (kept) SH_HIP(hipMemcpyAsync(out, buf.ptr, kept * sizeof(sahara_hit), hipMemcpyDeviceToDevice, st));
    return kept;
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
    size_t bytes = 0;
    SH_HIP(rocprim::radix_sort_pairs(nullptr, bytes, B.k0.ptr, B.k1.ptr, B.v0.ptr, B.v1.ptr, (size_t)n, 0, endBit, st));
    tmp.reserve(bytes + 256);
    SH_HIP(rocprim::radix_sort_pairs(tmp.ptr, bytes, B.k0.ptr, B.k1.ptr, B.v0.ptr, B.v1.ptr, (size_t)n, 0, endBit, st));
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

void launchPackPatterns3(const uint8_t* src, uint64_t npat, uint32_t m, uint32_t patBlocks, uint4* dst,
                         hipStream_t st) {
    const uint64_t blocks = std::min<uint64_t>((npat * patBlocks + 255) / 256, 65536);
    hipLaunchKernelGGL(kPackPatterns3, dim3((unsigned)blocks), dim3(256), 0, st, src, npat, m, patBlocks, dst);
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
