// search_fm.hip — search-scheme DFS on the GPU-resident FM-index (gfx950):
// the seeds and phase 1 of the search.
//
// Replaces fmc::search_ng24::search<Edit> (the reference's src/sahara/search.cpp:227,230)
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
// *text task* per row instead of being ranked further. The node step itself
// is fm_step.h, shared with host code.
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
// pairs whether it is ranked or split into its len occurrences
// (tests/fm_step_check.cpp holds both steps to that on the host).
//
// Leaves are compacted into the hit buffer with a wave ballot + prefix count
// into per-wave reserved slot ranges (one atomic per 64 slots). Overflow of
// any buffer is flagged; the host re-runs the batch with a larger buffer.
//
// Locate (locate_sort.hip): FM leaves resolve rows through the resident full
// SA (one read per row) or, in the reference mode, by LF walks to the SA
// samples, straight into per-query segments (counting sort by qid: row counts,
// exclusive scan). Keys text position << 4 | e are then sorted within each
// segment — in registers for the usual <= 8 rows, by a segmented radix sort
// for longer segments — for the canonical (qid, seq_id, pos, e) order.

#include <hip/hip_runtime.h>

#include "fm_step.h"
#include "search_device.h"

namespace sahara {
namespace {

__device__ __forceinline__ uint4 u4(const FmNode& n) { return make_uint4(n.x, n.y, n.z, n.w); }
__device__ __forceinline__ FmNode nodeOf(const uint4& v) { return {v.x, v.y, v.z, v.w}; }

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

// Pair-cooperative addressing: the two lanes of a pair read each other's
// records together, each lane one half of the even lane's record (E), then of
// the odd lane's (O), so that a load instruction touches at most 32 distinct
// lines (address translation, not bandwidth, bounds random lookups in a
// multi-GB table: tools/gather_bench). Must be called by all lanes.
struct PairAddr {
    uint64_t addrE, addrO;
    bool needE, needO;
};
__device__ __forceinline__ PairAddr pairAddr(uint64_t own, bool need, bool odd) {
    const uint64_t other = pairSwap64(own);
    const bool otherNeed = pairSwap(need ? 1u : 0u) != 0u;
    return {odd ? other : own, odd ? own : other, odd ? otherNeed : need, odd ? need : otherNeed};
}

// Pair-cooperative fetch of the rank part (bytes 0..47) of one 64-B Occ line
// per lane. Must be called by all 64 lanes (wave-uniform control flow):
// for the pair (E = even lane's line, O = odd lane's line) four loads run
//   #1 E bytes 0-15 | 16-31   #2 E bytes 32-47 | 48-63
//   #3 O bytes 0-15 | 16-31   #4 O bytes 32-47 | 48-63
// (even | odd lane); two DPP swaps then hand each lane the chunks of its own line.
__device__ __forceinline__ void fetchLinePair(uint64_t own, bool need, bool odd, uint32_t cnt[5], uint64_t p[3]) {
    const PairAddr pa = pairAddr(own, need, odd);
    const uint32_t half = odd ? 16u : 0u;
    uint4 r1 = make_uint4(0, 0, 0, 0), r2 = r1, r3 = r1, r4 = r1;
    if (pa.needE) {
        r1 = loadGlobal4(reinterpret_cast<const uint4*>(pa.addrE + half));
        r2 = loadGlobal4(reinterpret_cast<const uint4*>(pa.addrE + 32 + half));
    }
    if (pa.needO) {
        r3 = loadGlobal4(reinterpret_cast<const uint4*>(pa.addrO + half));
        r4 = loadGlobal4(reinterpret_cast<const uint4*>(pa.addrO + 32 + half));
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

__device__ __forceinline__ uint32_t nib(uint32_t word, uint32_t i) { return (word >> ((i & 7u) * 4u)) & 0xFu; }

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
// other's 16-B entries of the 68.7 GB table cooperatively (pairAddr): each
// lane 8 B of the even lane's entry, then 8 B of the odd lane's, swapped back
// with DPP. Must be called by all lanes of the wave.
template <int SIGMA>
__device__ __forceinline__ uint4 seedOf(const SeedArgs& a, uint32_t i, bool& keep, uint32_t& textPos, bool& skipped) {
    keep = i < a.nitems;
    // besthits: the pattern reported in an earlier round (nothing writes the
    // counts while the seeds run: pass.cpp issueFM)
    skipped = keep && a.skip && a.skip[i / a.nsearch] != 0u;
    keep = keep && !skipped;
    const uint32_t code = keep ? seedCode<SIGMA>(a, i) : ~0u;
    const bool need = keep && code != ~0u;
    const bool odd = (threadIdx.x & 1u) != 0u;
    const PairAddr pa = pairAddr((uint64_t)(a.kmer + (need ? code : 0u)), need, odd);
    const uint32_t half = odd ? 8u : 0u;
    uint2 rE = make_uint2(0u, 0u), rO = rE;
    if (pa.needE) rE = *reinterpret_cast<const uint2*>(pa.addrE + half);  // even's entry: bytes 0-7 | 8-15
    if (pa.needO) rO = *reinterpret_cast<const uint2*>(pa.addrO + half);  // odd's entry: bytes 0-7 | 8-15
    const uint2 gE = make_uint2(pairSwap(rE.x), pairSwap(rE.y));           // even <- bytes 8-15 of its entry
    const uint2 gO = make_uint2(pairSwap(rO.x), pairSwap(rO.y));           // odd <- bytes 0-7 of its entry
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
            if (task[k]) {  // the seed's one row, or its text position (kTaskPos)
                const uint32_t at = tslot + (uint32_t)__popcll(mt[k] & ltMask);
                const uint32_t pid = item / a.nsearch, sIdx = item - pid * a.nsearch;
                if (at < a.taskCap)
                    a.tasks[at] = u4(taskRecord(a.kmerPos ? tpos[k] : cur[k].x, a.kmerPos != 0u, nodeOf(cur[k]), pid, sIdx));
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

// What a lane works on: its item (pattern, search) and its DFS state: a node
// in registers and the stack entries [bot, sp).
struct FmLane {
    uint32_t pid = 0, sIdx = 0;
    FmNode cur = {0, 0, 0, 0};
    uint32_t sp = 0, bot = 0;
    bool have = false;
    __device__ __forceinline__ bool idle() const { return !have && sp == bot; }
};

// ---- the seed feed: seeds (kSeedItems: starting cursor + item) arrive from a
// striped queue in chunks of kSeedChunk, one record per lane, prefetched a
// chunk ahead so a refill costs no memory trip. (The text kernel's TaskFeed is
// the same construct over one-word-less records with an SA resolve on top; the
// two stay separate types, so that neither kernel carries the other's state.)
struct SeedFeed {
    const SearchArgs& a;
    StripedQueue queue;
    uint4 curRec = make_uint4(0, 0, 0, 0), nextRec = make_uint4(0, 0, 0, 0);
    uint32_t curItem = 0, nextItem = 0, nBase = 0, nEnd = 0, qBase = 0, qNext = 0, qEnd = 0;
    bool haveNext = false, qDone = false;

    __device__ __forceinline__ SeedFeed(const SearchArgs& args, uint32_t lane) : a(args), queue(args.work, *args.seedCount) {
        prefetch(lane);
    }
    // grab the next chunk off the queue and start reading its records (wave-uniform)
    __device__ __forceinline__ void prefetch(uint32_t lane) {
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
    __device__ __forceinline__ bool chunkEmpty() const { return qNext >= qEnd; }
    // no seed left, now or later (wave-uniform)
    __device__ __forceinline__ bool dry() const { return qDone && !haveNext && qNext >= qEnd; }
    // the prefetched chunk becomes current, the one after it is prefetched (haveNext)
    __device__ __forceinline__ void advance(uint32_t lane) {
        qBase = nBase;
        qNext = nBase;
        qEnd = nEnd;
        curRec = nextRec;
        curItem = nextItem;
        haveNext = false;
        if (!qDone) prefetch(lane);
    }
    // hand the current chunk's next records to the lanes of `pending`, lowest
    // lane first; returns whether this lane got one (seed, item)
    __device__ __forceinline__ bool take(uint64_t pending, uint32_t lane, uint64_t ltMask, uint4& seed, uint32_t& item) {
        const uint32_t n = min(qEnd - qNext, (uint32_t)__popcll(pending));
        const uint32_t rank = (uint32_t)__popcll(pending & ltMask);
        const bool mine = ((pending >> lane) & 1ull) && rank < n;
        const uint32_t src = (qNext - qBase + rank) & 63u;
        seed = make_uint4(__shfl(curRec.x, src), __shfl(curRec.y, src), __shfl(curRec.z, src), __shfl(curRec.w, src));
        item = __shfl(curItem, src);
        qNext += n;
        return mine;
    }
};

// ---- a lane's DFS stack: entries [bot, sp) in a ring of `levels` levels
// (entry d at level d mod levels; bot < levels): pushes and pops at sp, work
// stealing takes the bottom entry (bot++). The bottom ldsDepth levels live in
// LDS after the scheme table ([level][thread], conflict-free 16-B rows when
// lanes sit at equal depth), deeper levels spill to HBM ([level][grid thread]).
struct FmStack {
    const SearchArgs& a;
    uint4* lstk;  // LDS levels
    uint4* gstk;  // HBM levels, this thread's column
    uint32_t ldsDepth, levels, T, gtid;
    __device__ __forceinline__ FmStack(const SearchArgs& args, uint32_t* sch)
        : a(args), lstk(reinterpret_cast<uint4*>(sch + ((args.nsearch * args.m + 3u) & ~3u))),
          gstk(args.stack + blockIdx.x * blockDim.x + threadIdx.x), ldsDepth(args.ldsDepth), levels(args.stackLevels),
          T(gridDim.x * blockDim.x), gtid(blockIdx.x * blockDim.x + threadIdx.x) {}
    __device__ __forceinline__ uint32_t level(uint32_t d) const { return d >= levels ? d - levels : d; }
    __device__ __forceinline__ uint4 get(uint32_t d) const {
        d = level(d);
        return d < ldsDepth ? lstk[d * 256u + threadIdx.x] : gstk[(size_t)(d - ldsDepth) * T];
    }
    __device__ __forceinline__ void put(uint32_t d, const uint4& v) const {
        d = level(d);
        if (d < ldsDepth) lstk[d * 256u + threadIdx.x] = v;
        else gstk[(size_t)(d - ldsDepth) * T] = v;
    }
    // a push past the DFS bound cannot happen (fm_step.h); flagged, not handled
    __device__ __forceinline__ void push(uint32_t& sp, uint32_t bot, const FmNode& v) const {
        if (sp - bot < a.stackCap) {
            put(sp, u4(v));
            ++sp;
        } else {
            atomicOr(a.flags, kFlagStack);
        }
    }
    __device__ __forceinline__ void pop(FmLane& ln) const {
        --ln.sp;
        ln.cur = nodeOf(get(ln.sp));
        ln.have = true;
    }
    // the bottom entry (level lv < levels) of lane `donor` of this wave
    __device__ __forceinline__ uint4 readBottomOf(uint32_t donor, uint32_t lv) const {
        if (lv < ldsDepth) return lstk[lv * 256u + ((threadIdx.x & ~63u) | donor)];
        return loadGlobal4(a.stack + (size_t)(lv - ldsDepth) * T + (gtid & ~63u) + donor);
    }
    __device__ __forceinline__ void dropBottom(FmLane& ln) const {
        if (++ln.bot == levels) {
            ln.bot = 0;
            ln.sp -= levels;
        }
    }
};

// ---- refill idle lanes from the wave's current seed chunk; returns whether
// this lane wanted a seed (all lanes call it)
__device__ __forceinline__ bool refillStage(FmLane& ln, SeedFeed& feed, bool exhausted, uint32_t nsearch, uint32_t lane,
                                            uint64_t ltMask) {
    const bool need = ln.idle() && !exhausted;
    uint64_t pending = __ballot(need);
    while (pending) {  // wave-uniform
        if (feed.chunkEmpty()) {
            if (!feed.haveNext) break;
            feed.advance(lane);
            if (feed.chunkEmpty()) continue;
        }
        uint4 seed;
        uint32_t item;
        const bool mine = feed.take(pending, lane, ltMask, seed, item);
        if (mine) {
            ln.pid = item / nsearch;
            ln.sIdx = item - ln.pid * nsearch;
            ln.cur = nodeOf(seed);
            ln.have = true;
        }
        pending &= ~__ballot(mine);
    }
    return need;
}

// ---- work stealing inside the wave once the seed queue is dry (wave-uniform
// call). The DFS of one seed varies by orders of magnitude in size (repeats,
// and from the root every search ranks thousands of nodes at k = 3), so a
// launch otherwise ends with most lanes idle beside a few long ones
// (reference execution at C5: lanes busy 0.49). An idle lane takes the bottom
// (shallowest, so largest) stack entry of the r-th busy lane, with its pattern
// id and search by shuffle; the entry's subtree is the same DFS whichever lane
// runs it, so the leaves are too.
__device__ __forceinline__ void stealStage(FmLane& ln, const FmStack& stack, uint32_t stealAt, uint32_t lane,
                                           uint64_t ltMask) {
    const StealPlan p = stealPlan(!ln.have, ln.have && ln.sp > ln.bot, stealAt, lane, ltMask);
    if (!p.any) return;  // wave-uniform
    const uint32_t dPid = __shfl(ln.pid, p.donor), dS = __shfl(ln.sIdx, p.donor), dBot = __shfl(ln.bot, p.donor);
    if (p.takes) {
        ln.cur = nodeOf(stack.readBottomOf(p.donor, dBot));
        ln.pid = dPid;
        ln.sIdx = dS;
        ln.have = true;
    }
    p.settle();  // before a donor's later pushes can reuse the level (its stack emptied and reset)
    if (p.gives) stack.dropBottom(ln);
}

// ---- leaves -> hit buffer, each ranked in its query's segment as it is
// written; returns the hits this lane wrote (all lanes call it)
__device__ __forceinline__ uint32_t leafStage(FmLane& ln, SlotRange& slots, const SearchArgs& a, uint32_t lane,
                                              uint64_t ltMask) {
    const bool leaf = ln.have && fmIsLeaf(ln.cur, a.m);
    uint32_t slot;
    if (!(slots.take(leaf, lane, ltMask, a.hitCount, slot) && leaf)) return 0u;
    if (slot < a.hitCap) {
        a.hits[slot] = u4(fmHit(ln.pid, ln.cur));
        a.rank[slot] = atomicAdd(a.qcnt + ln.pid, ln.cur.z);  // its first row's place in the query's segment
    } else {
        atomicOr(a.flags, kFlagHits);
    }
    ln.have = false;
    return 1u;
}

// ---- small intervals -> one text task per row (phase 2); returns the tasks
// this lane wrote (all lanes call it)
__device__ __forceinline__ uint32_t convertStage(FmLane& ln, SlotRange& slots, const SearchArgs& a, uint32_t lane,
                                                 uint64_t ltMask) {
    const bool conv = ln.have && fmConverts(ln.cur, a.split);
    uint32_t written = 0;
    for (uint32_t j = 0; __any(conv && j < ln.cur.z); ++j) {  // wave-uniform trip count
        const bool want = conv && j < ln.cur.z;
        uint32_t slot;
        if (slots.take(want, lane, ltMask, a.taskCount, slot) && want) {
            if (slot < a.taskCap) a.tasks[slot] = u4(taskRecord(ln.cur.x + j, false, ln.cur, ln.pid, ln.sIdx));
            else atomicOr(a.flags, kFlagTasks);
            ++written;
        }
    }
    if (conv) ln.have = false;
    return written;
}

// ---- instrumentation (count mode only; the product variants get the empty form)
template <bool COUNT>
struct FmProbe {
    __device__ __forceinline__ void iteration(uint32_t) {}
    __device__ __forceinline__ void tasks(uint32_t) {}
    __device__ __forceinline__ void node(const FmDecode&) {}
    __device__ __forceinline__ void flush(const SearchArgs&) {}
};
template <>
struct FmProbe<true> {
    uint64_t cNodes = 0, cRank = 0, cLines = 0, cTasks = 0, cIter = 0;
    __device__ __forceinline__ void iteration(uint32_t lane) { cIter += lane == 0 ? 1u : 0u; }
    __device__ __forceinline__ void tasks(uint32_t n) { cTasks += n; }
    __device__ __forceinline__ void node(const FmDecode& d) {
        ++cNodes;
        if (d.needA) { ++cRank; cLines += d.needB ? 2 : 1; }
    }
    __device__ __forceinline__ void flush(const SearchArgs& a) {
        atomicAdd(a.counters + kCtNodes, (unsigned long long)cNodes);
        atomicAdd(a.counters + kCtRankNodes, (unsigned long long)cRank);
        atomicAdd(a.counters + kCtExtLines, (unsigned long long)cLines);
        atomicAdd(a.counters + kCtTextTasks, (unsigned long long)cTasks);
        if (cIter) atomicAdd(a.counters + kCtFmIter, (unsigned long long)cIter);
    }
};

// ---- kSearchFM: the FM phase of one batch. Per iteration, a wave
//   refills its idle lanes with seeds, or pops their stacks,
//   steals inside the wave once the seed queue is dry,
//   emits the leaves among its nodes as hits and hands small intervals on as text tasks,
//   decodes each lane's node, fetches the nodes' Occ lines pair-cooperatively
//   and expands the children (fm_step.h).
template <int SIGMA, bool EDIT, bool COUNT>
__global__ __launch_bounds__(256) void kSearchFM(SearchArgs a) {
    extern __shared__ uint32_t sch[];
    for (uint32_t i = threadIdx.x; i < a.nsearch * a.m; i += blockDim.x) sch[i] = a.scheme[i];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ltMask = (1ull << lane) - 1ull;
    const bool odd = lane & 1u;
    const FmStack stack(a, sch);
    FmLane ln;
    bool exhausted = false;
    uint32_t filled = 0;
    SlotRange hitSlots, taskSlots;
    SeedFeed feed(a, lane);
    FmProbe<COUNT> probe;

    for (;;) {
        const bool need = refillStage(ln, feed, exhausted, a.nsearch, lane, ltMask);
        exhausted = exhausted || (feed.dry() && need && !ln.have);
        if (!ln.have && ln.sp > ln.bot) stack.pop(ln);
        if (ln.sp == ln.bot) ln.sp = ln.bot = 0;
        if (a.stealAt && feed.dry()) stealStage(ln, stack, a.stealAt, lane, ltMask);
        if (!__any(ln.have)) break;
        probe.iteration(lane);

        filled += leafStage(ln, hitSlots, a, lane, ltMask);
        if (a.split) probe.tasks(convertStage(ln, taskSlots, a, lane, ltMask));

        // ---- first half of the step (per lane); an idle lane fetches nothing
        uint32_t se = 0, cq = 0;
        if (ln.have) {
            se = sch[ln.sIdx * a.m + ln.cur.pos()];
            const uint32_t q = schemeQ(se);
            cq = nib(a.pats[(size_t)ln.pid * a.patWords + (q >> 3)], q);
        }
        const FmDecode d = fmDecode<EDIT>(ln.cur, se, cq, ln.have);
        // ---- pair-cooperative Occ line fetch (wave-uniform)
        const uint64_t occ = (uint64_t)(d.right ? a.occR : a.occF);
        uint32_t ca[5], cb[5];
        uint64_t pa[3], pb[3];
        fetchLinePair(occ + (uint64_t)(d.lo >> 6) * 64u, d.needA, odd, ca, pa);
        fetchLinePair(occ + (uint64_t)(d.hi >> 6) * 64u, d.needB, odd, cb, pb);
        // ---- second half: rank, update, children
        if (ln.have) {
            probe.node(d);
            FmNode next;
            uint32_t sp = ln.sp;
            const uint32_t bot = ln.bot;
            uint32_t C[SIGMA];  // copied here, not held in SGPRs across the loop (which spilled others)
#pragma unroll
            for (int c = 0; c < SIGMA; ++c) C[c] = a.C[c];
            ln.have = fmExpand<SIGMA>(ln.cur, d, ca, pa, cb, pb, C, [&](const FmNode& v) { stack.push(sp, bot, v); }, next);
            ln.cur = next;
            ln.sp = sp;
        }
    }
    hitSlots.close(lane, a.hits, a.hitCap);
    taskSlots.close(lane, a.tasks, a.taskCap);
    if (filled) atomicAdd(a.filled, filled);  // per-lane counts
    probe.flush(a);
}

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

}  // namespace sahara
