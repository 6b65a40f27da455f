// search_text.hip — phase 2 of the search (search_fm.hip has the overview): the
// text tasks of one batch, each a DFS node whose string occurs once, expanded
// against the text itself in LDS (gfx950).
//
// LDS: table[S*m] (TextRow, text_step.h) | per lane, interleaved so that the
// lanes of a wave hit consecutive banks at equal offsets:
//   window  (winBlocks blocks of 32 symbols)     W[(3j+b)*256 + t], plane b
//   pattern (patBlocks blocks of 32 symbols)     P[(3j+b)*256 + t]
//   stack   (stackCap entries)                   S[d*256 + t]: a TextNode
//
// A lane's state is one DFS node and its stack. Every micro-step
// (text_step.h: textStep) is straight-line code — one stack read, one table
// read, one 32-symbol read each of the window beyond the span and of the
// pattern from pi[pos], the stack writes of the surviving children — so the
// lanes of a wave stay converged. A node with e == u[pos] takes up to kRun
// forced matches at once, a node one error below its bound walks up to kChain
// positions of its match chain: the DFS visits the same nodes, one micro-step
// per run or chain.

#include <hip/hip_runtime.h>

#include "fm_step.h"
#include "search_device.h"
#include "text_step.h"

namespace sahara {
namespace {

// 32 symbols from offset o of a lane's interleaved plane array (block i, plane
// b at word (3i + b) * 256). o may be negative (down to -32): reads may run
// past either end of the array into the lane's neighbouring LDS regions; callers
// mask.
__device__ __forceinline__ uint32_t read32(const uint32_t* A, int o, uint32_t b) {
    const int i = o >> 5;
    return __builtin_amdgcn_alignbit(A[(3 * i + 3 + (int)b) * 256], A[(3 * i + (int)b) * 256], (uint32_t)o & 31u);
}
// 32 symbols in chain order: right (fwd) from o, or left ending at o - 1 and
// reversed (back: bit j = symbol o - 1 - j). Symbols outside the array are
// whatever the LDS holds there (the window's block -1 is the table region,
// kTextTableMin words, the pattern's is the window): the window's are masked
// by textStep's `avail`, the pattern's lie beyond the pattern, which the chain
// logic never uses (tests/text_step_check.cpp reads arbitrary symbols there).
__device__ __forceinline__ Planes chain32(const uint32_t* A, uint32_t o, bool fwd) {
    const int off = (int)o - (fwd ? 0 : 32);
    Planes r;
    uint32_t v[3];
#pragma unroll
    for (uint32_t b = 0; b < 3; ++b) {
        const uint32_t w = read32(A, off, b);
        v[b] = fwd ? w : __builtin_bitreverse32(w);
    }
    r.b0 = v[0]; r.b1 = v[1]; r.b2 = v[2];
    return r;
}

// Raw buffer resource over [base, base + bytes) (gfx9 dword3): loads at an
// offset past the end return 0 without a memory request, so guarded loads
// need no branch (and no wait at a branch join).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bufferOf(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
constexpr uint32_t kBufOOB = 0xFFFFFFFFu;  // offset of a load that returns 0

// Copy two block arrays (window, pattern) from global memory into this lane's
// interleaved LDS slots (3 words per block): all loads of up to 8 blocks of
// each array are issued before the first store, so a task start costs one
// memory round trip for m <~ 190.
__device__ __forceinline__ void copyBlocks(uint32_t* DA, __amdgpu_buffer_rsrc_t RA, uint32_t offA, uint32_t na,
                                           uint32_t* DB, __amdgpu_buffer_rsrc_t RB, uint32_t offB, uint32_t nb) {
    const uint32_t n = max(na, nb);
    for (uint32_t c = 0; c < n; c += 8) {
        decltype(__builtin_amdgcn_raw_buffer_load_b128(RA, 0u, 0, 0)) va[8], vb[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t j = c + i;
            va[i] = __builtin_amdgcn_raw_buffer_load_b128(RA, j < na ? offA + 16u * j : kBufOOB, 0, 0);
            vb[i] = __builtin_amdgcn_raw_buffer_load_b128(RB, j < nb ? offB + 16u * j : kBufOOB, 0, 0);
        }
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t j = c + i;
            if (j < na) { uint32_t* D = DA + 3u * j * 256u; D[0] = va[i][0]; D[256] = va[i][1]; D[512] = va[i][2]; }
            if (j < nb) { uint32_t* D = DB + 3u * j * 256u; D[0] = vb[i][0]; D[256] = vb[i][1]; D[512] = vb[i][2]; }
        }
    }
}

// Same, but the window starts at any symbol: na blocks come from na + 1
// source blocks funnel-shifted by sh symbols (na + 1 <= 8, nb <= 8).
__device__ __forceinline__ void copyBlocksShifted(uint32_t* DA, __amdgpu_buffer_rsrc_t RA, uint32_t offA, uint32_t sh,
                                                  uint32_t na, uint32_t* DB, __amdgpu_buffer_rsrc_t RB, uint32_t offB,
                                                  uint32_t nb) {
    decltype(__builtin_amdgcn_raw_buffer_load_b128(RA, 0u, 0, 0)) va[8], vb[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        va[j] = __builtin_amdgcn_raw_buffer_load_b128(RA, j <= na ? offA + 16u * j : kBufOOB, 0, 0);
        vb[j] = __builtin_amdgcn_raw_buffer_load_b128(RB, j < nb ? offB + 16u * j : kBufOOB, 0, 0);
    }
#pragma unroll
    for (uint32_t j = 0; j < 7; ++j)
        if (j < na) {
            uint32_t* D = DA + 3u * j * 256u;
            D[0] = __builtin_amdgcn_alignbit(va[j + 1][0], va[j][0], sh);
            D[256] = __builtin_amdgcn_alignbit(va[j + 1][1], va[j][1], sh);
            D[512] = __builtin_amdgcn_alignbit(va[j + 1][2], va[j][2], sh);
        }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
        if (j < nb) { uint32_t* D = DB + 3u * j * 256u; D[0] = vb[j][0]; D[256] = vb[j][1]; D[512] = vb[j][2]; }
}

// SHAPE fixes the window and pattern block counts at compile time, so that
// the task-start copy is straight-line code with no per-block conditions (the
// generic form, SHAPE 0, keeps ~30 block masks in spilled SGPRs and reloads
// them at every task start: 1882 against 1311 instructions, 101 against 85
// VGPRs; C3 850-863M -> 886-893M reads/s).
//   1: window 4 blocks at an exact start, pattern 4 blocks (C2, C3: m = 100)
//   2: window 9 blocks block-aligned, pattern 8 blocks (C5: m = 250, k = 3)
struct TextShape { uint32_t win, pat; bool exact; };
constexpr int kTextShapes = 3;
__host__ __device__ constexpr TextShape textShape(int shape) {
    return shape == 1 ? TextShape{4, 4, true} : shape == 2 ? TextShape{9, 8, false} : TextShape{0, 0, false};
}

// A lane's regions of the block's LDS, and the geometry they follow from.
struct LaneLds {
    const uint2* table;  // the scheme's rows
    uint32_t* slot;      // the lanes' interleaved regions; this lane's words are slot[k * 256 + threadIdx.x]
    uint32_t* W;         // window
    uint32_t* P;         // pattern
    uint2* S;            // stack
    uint32_t winBlocks, patBlocks;
    bool exactWindow;
    __device__ __forceinline__ TextRow row(uint32_t i) const { const uint2 v = table[i]; return {v.x, v.y}; }
    __device__ __forceinline__ TextNode stackGet(uint32_t d) const { const uint2 v = S[d * 256u]; return {v.x, v.y}; }
    __device__ __forceinline__ void stackPut(uint32_t d, const TextNode& n) const { S[d * 256u] = make_uint2(n.x, n.y); }
    __device__ __forceinline__ uint32_t copyWords() const { return 3u * (winBlocks + patBlocks); }  // window + pattern
};

// What a lane works on: its task (pattern, window start in the text, first
// table row of its search) and its DFS state (a node in registers, sp stack
// entries in LDS).
struct TextLane {
    uint32_t pid = 0, wb = 0, sBase = 0;
    TextNode cur = {0, 0};
    uint32_t sp = 0;
    bool have = false;
    __device__ __forceinline__ bool busy() const { return have || sp > 0; }
};

// ---- the task feed: the launch's tasks come from a striped queue in chunks
// of kTaskChunk records, one per lane: the current chunk's and the next one's,
// prefetched a chunk ahead so that a refill needs no dependent task read.
struct TaskFeed {
    StripedQueue queue;
    const uint4* tasks;
    const uint32_t* sa;
    uint4 curRec = make_uint4(0, 0, 0, 0), nextRec = make_uint4(0, 0, 0, 0);
    uint32_t nBase = 0, nEnd = 0, qBase = 0, qNext = 0, qEnd = 0;
    bool haveNext = false, qDone = false;
    // The prefetched chunk's records still hold SA rows. Their text positions
    // are read at the next refill, beside its window loads (one round trip for
    // both), or at the latest when the chunk becomes current.
    bool nextRaw = false;

    __device__ __forceinline__ TaskFeed(uint32_t* work, const uint4* t, uint32_t ntasks, const uint32_t* s, uint32_t lane)
        : queue(work, ntasks), tasks(t), sa(s) {
        prefetch(lane);
    }
    // grab the next chunk off the queue and start reading its records (wave-uniform)
    __device__ __forceinline__ void prefetch(uint32_t lane) {
        uint32_t b = 0, e = 0;
        if (!queue.next(lane, kTaskChunk, b, e)) {
            qDone = true;
        } else {
            nBase = b;
            nEnd = e;
            if (b + lane < e) nextRec = tasks[b + lane];
            haveNext = true;
            nextRaw = true;
        }
    }
    __device__ __forceinline__ void resolveNext(uint32_t lane) {
        if (nextRaw) {  // wave-uniform
            if (nBase + lane < nEnd && !(nextRec.y & kTaskPos)) nextRec.x = sa[nextRec.x];
            nextRaw = false;
        }
    }
    __device__ __forceinline__ bool chunkEmpty() const { return qNext >= qEnd; }
    // no task left, now or later (wave-uniform)
    __device__ __forceinline__ bool dry() const { return qDone && !haveNext && qNext >= qEnd; }
    // the prefetched chunk becomes current, the one after it is prefetched (haveNext)
    __device__ __forceinline__ void advance(uint32_t lane) {
        resolveNext(lane);
        qBase = nBase;
        qNext = nBase;
        qEnd = nEnd;
        curRec = nextRec;
        haveNext = false;
        if (!qDone) prefetch(lane);
    }
    // hand the current chunk's next records to the lanes of `pending`, lowest
    // lane first; returns whether this lane got one (t). The records sit one
    // per lane: each lane fetches its own by shuffle.
    __device__ __forceinline__ bool take(uint64_t pending, uint32_t lane, uint64_t ltMask, uint4& t) {
        const uint32_t n = min(qEnd - qNext, (uint32_t)__popcll(pending));
        const uint32_t rank = (uint32_t)__popcll(pending & ltMask);
        const bool mine = ((pending >> lane) & 1ull) && rank < n;
        const uint32_t srcLane = (qNext - qBase + rank) & 63u;
        t = make_uint4(__shfl(curRec.x, srcLane), __shfl(curRec.y, srcLane), __shfl(curRec.z, srcLane),
                       __shfl(curRec.w, srcLane));
        qNext += n;
        return mine;
    }
};

// ---- start a task (record rec, fm_step.h taskRecord, its x a text position
// by now): copy the pattern and the text window that its subtree can reach
// into the lane's LDS
__device__ __forceinline__ void startTask(TextLane& ln, const uint4& rec, const LaneLds& L, uint32_t m,
                                          __amdgpu_buffer_rsrc_t textBuf, __amdgpu_buffer_rsrc_t patBuf) {
    const TextTask t = taskOf({rec.x, rec.y, rec.z, rec.w});
    const uint32_t x = t.x;
    ln.pid = t.pid;
    ln.sBase = t.search * m;
    const uint32_t meta = t.meta;
    const uint32_t pos = meta & 0xFFFFu, e = (meta >> 16) & 0xFu;
    const uint32_t ca = L.row(ln.sBase + pos).coverBegin();
    const uint32_t K = L.row(ln.sBase + m - 1u).ub();
    const uint32_t left = ca + (K > e ? K - e : 0u);  // text the left side can still consume
    uint32_t wb = x > left ? x - left : 0u;           // window start
    if (L.exactWindow) {  // at wb: m + 2k symbols fit in winBlocks blocks
        copyBlocksShifted(L.W, textBuf, (wb >> 5) * 16u, wb & 31u, L.winBlocks, L.P, patBuf,
                          ln.pid * L.patBlocks * 16u, L.patBlocks);
    } else {              // at the block start below wb (31 more symbols)
        wb &= ~31u;
        copyBlocks(L.W, textBuf, (wb >> 5) * 16u, L.winBlocks, L.P, patBuf, ln.pid * L.patBlocks * 16u, L.patBlocks);
    }
    ln.wb = wb;
    ln.cur = textNode(x - wb, x + t.tlen - wb, meta);
    ln.have = true;
}

// ---- work stealing inside the wave once the task queue is dry (wave-uniform
// call). A launch ends on its longest subtrees, each on one lane while the
// others idle (C5: lanes busy 0.655 of the time); an idle lane takes the
// bottom (shallowest, so largest) stack entry of a busy lane, with that lane's
// window and pattern copied slot to slot in LDS, and the task state (pattern
// id, window start, scheme row) by shuffle. The DFS of the entry is the same
// whichever lane runs it, so the hits are too. Returns whether this lane took
// a node.
__device__ __forceinline__ bool stealStage(TextLane& ln, const LaneLds& L, uint32_t stealAt, uint32_t lane,
                                           uint64_t ltMask) {
    const StealPlan p = stealPlan(!ln.have && ln.sp == 0u, ln.sp >= 2u || (ln.sp == 1u && ln.have), stealAt, lane, ltMask);
    if (!p.any) return false;  // wave-uniform
    const uint32_t dPid = __shfl(ln.pid, p.donor), dWb = __shfl(ln.wb, p.donor), dBase = __shfl(ln.sBase, p.donor);
    const uint32_t dTid = (threadIdx.x & ~63u) | p.donor;
    if (p.takes) {
        const uint32_t* src = L.slot + dTid;
        uint32_t* dst = L.slot + threadIdx.x;
        for (uint32_t k = 0; k < L.copyWords(); ++k) dst[k * 256u] = src[k * 256u];
        const uint2 node = reinterpret_cast<const uint2*>(L.slot + L.copyWords() * 256u)[dTid];  // the donor's S[0]
        ln.cur = {node.x, node.y};
        ln.pid = dPid;
        ln.wb = dWb;
        ln.sBase = dBase;
        ln.have = true;
    }
    p.settle();
    if (p.gives) {  // donors drop their bottom entry
        for (uint32_t d = 1; d < ln.sp; ++d) L.stackPut(d - 1u, L.stackGet(d));
        --ln.sp;
    }
    return p.takes;
}

// ---- hit emission: leaves are hits (qid, text position, 1, e | kPosKnown)
// in per-wave reserved slots, each ranked in its query's segment (a.qcnt, the
// FM phase's counts) as it is written. The atomic's result is stored at the
// lane's next emission, so that its round trip overlaps the micro-steps in
// between (kLocate then places the hit without an atomic of its own).
struct HitWriter {
    SlotRange slots;
    uint32_t rankSlot = ~0u, rankVal = 0;  // the lane's last hit whose rank is not stored yet
    uint32_t filled = 0;
    // all lanes call it (wave-uniform)
    __device__ __forceinline__ void emit(const TextBatchArgs& a, bool leaf, uint32_t lane, uint64_t ltMask, uint32_t pid,
                                         uint32_t pos, uint32_t e) {
        uint32_t s;
        if (slots.take(leaf, lane, ltMask, a.hitCount, s) && leaf) {
            if (s < a.hitCap) {
                a.hits[s] = make_uint4(pid, pos, 1u, e | kPosKnown);
                if (rankSlot != ~0u) a.rank[rankSlot] = rankVal;
                rankVal = atomicAdd(a.qcnt + pid, 1u);
                rankSlot = s;
            } else {
                atomicOr(a.flags, kFlagHits);
            }
            ++filled;
        }
    }
    __device__ __forceinline__ void finish(const TextBatchArgs& a, uint32_t lane) {
        slots.close(lane, a.hits, a.hitCap);
        if (rankSlot != ~0u) a.rank[rankSlot] = rankVal;
        if (filled) atomicAdd(a.filled, filled);  // per-lane counts
    }
};

// ---- instrumentation (count mode only: the product variants get the empty
// form and pay nothing; the probe alone would cost them 14 VGPRs and 12 SGPR
// spills). Work counters and cycles per stage of every launch, and — with
// a.probe — the waves' lives on the wall clock: born, the queue seen drained,
// iterations and busy lanes before / after it (flushed for the pass's first
// launch, a.isFirst).
template <bool COUNT>
struct TextProbe {
    __device__ __forceinline__ TextProbe(const TextBatchArgs&, uint32_t, uint64_t*) {}
    __device__ __forceinline__ void iterBegin() {}
    __device__ __forceinline__ void refilled(bool, bool, bool) {}
    __device__ __forceinline__ void stolen(bool) {}
    __device__ __forceinline__ void stepped(const TextStepResult&) {}
    __device__ __forceinline__ void stepsDone() {}
    __device__ __forceinline__ void emitted(bool) {}
    __device__ __forceinline__ void flush() {}
};
template <>
struct TextProbe<true> {
    const TextBatchArgs& a;
    const uint32_t lane;
    const bool wall;            // a.probe
    uint64_t* born;             // this wave's {born, drained} wall clock, in LDS
    uint64_t cNodes = 0, cCmp = 0, cSteps = 0, cSteal = 0;   // per lane
    uint64_t tIter = 0, tActive = 0, tRefill = 0;            // lane 0
    uint64_t cyRefill = 0, cyStep = 0, cyEmit = 0, t0 = 0;
    uint32_t pIterPre = 0, pIterPost = 0, pActPre = 0, pActPost = 0;
    uint64_t pwPreA = 0, pwPreB = 0, pwPostA = 0, pwPostB = 0, pw0 = 0, pw1 = 0;

    __device__ __forceinline__ TextProbe(const TextBatchArgs& args, uint32_t l, uint64_t* waveClock)
        : a(args), lane(l), wall(args.probe != 0u), born(waveClock + 2u * (threadIdx.x >> 6)) {
        if (wall && lane == 0) born[0] = wall_clock64(), born[1] = 0;
    }
    __device__ __forceinline__ void iterBegin() {
        if (wall) pw0 = wall_clock64();
        t0 = clock64();
    }
    // after the refill and steal stages: `active` = the lane is busy (all lanes call it)
    __device__ __forceinline__ void refilled(bool qDone, bool active, bool refill) {
        const uint32_t act = (uint32_t)__popcll(__ballot(active));
        if (wall) {
            if (qDone && lane == 0 && born[1] == 0) born[1] = wall_clock64();
            if (qDone) { ++pIterPost; pActPost += act; } else { ++pIterPre; pActPre += act; }
            pw1 = wall_clock64();
        }
        if (lane == 0) { ++tIter; tActive += act; tRefill += refill ? 1u : 0u; }
        const uint64_t t1 = clock64();
        cyRefill += t1 - t0;
        t0 = t1;
    }
    __device__ __forceinline__ void stolen(bool took) { cSteal += took ? 1u : 0u; }
    __device__ __forceinline__ void stepped(const TextStepResult& r) {
        cNodes += r.nodes;
        cCmp += r.compares;
        cSteps += r.steps;
    }
    __device__ __forceinline__ void stepsDone() {
        const uint64_t t1 = clock64();
        cyStep += t1 - t0;
        t0 = t1;
    }
    __device__ __forceinline__ void emitted(bool qDone) {
        cyEmit += clock64() - t0;
        if (wall) {
            const uint64_t pw2 = wall_clock64();
            if (qDone) { pwPostA += pw1 - pw0; pwPostB += pw2 - pw1; }
            else { pwPreA += pw1 - pw0; pwPreB += pw2 - pw1; }
        }
    }
    __device__ __forceinline__ void add(uint32_t counter, uint64_t v) {
        atomicAdd(a.counters + counter, (unsigned long long)v);
    }
    __device__ __forceinline__ void flush() {
        if (wall && a.isFirst && lane == 0) {
            const uint64_t wEnd = wall_clock64(), w0 = born[0], wd = born[1];
            atomicMin(a.counters + kCtBornMin, (unsigned long long)w0);
            atomicMax(a.counters + kCtBornMax, (unsigned long long)w0);
            atomicMax(a.counters + kCtEndMax, (unsigned long long)wEnd);
            add(kCtLifeSum, wEnd - w0);
            atomicMin(a.counters + kCtEndMin, (unsigned long long)wEnd);
            if (wd) {
                atomicMin(a.counters + kCtDryMin, (unsigned long long)wd);
                atomicMax(a.counters + kCtDryMax, (unsigned long long)wd);
                add(kCtDryRun, wEnd - wd);
                add(kCtDryWaves, 1);
            }
            add(kCtIterPre, pIterPre);
            add(kCtActPre, pActPre);
            add(kCtIterPost, pIterPost);
            add(kCtActPost, pActPost);
            add(kCtWallPreRefill, pwPreA);
            add(kCtWallPreStep, pwPreB);
            add(kCtWallPostRefill, pwPostA);
            add(kCtWallPostStep, pwPostB);
        }
        add(kCtTextNodes, cNodes);
        if (lane == 0) {
            add(kCtTextIter, tIter);
            add(kCtTextActive, tActive);
            add(kCtTextRefills, tRefill);
            add(kCtCyRefill, cyRefill);
            add(kCtCyStep, cyStep);
            add(kCtCyEmit, cyEmit);
        }
        add(kCtCompareSteps, cCmp);
        add(kCtTextSteps, cSteps);
        if (cSteal) add(kCtStolen, cSteal);
    }
};

// ---- kSearchTextBatch: the text phase of one batch per launch. Its tasks
// [*taskBegin, *taskCount) of the slot's list come from a striped queue. Per
// iteration, a wave
//   refills its idle lanes in batches: a lane takes a task (text position, or
//     SA row read here) and copies the window and pattern to LDS,
//   steals inside the wave once the queue is dry,
//   runs up to a.steps micro-steps of each lane's DFS against the text, and
//   emits the leaves reached as hits.
// (Round 5's persistent variant, one launch per pass, measured 2-3x slower and
// was removed in r6: DESIGN.md §3.4.)
template <bool EDIT, bool COUNT, int SHAPE>
__global__ __launch_bounds__(256) void kSearchTextBatch(TextBatchArgs a) {
    extern __shared__ uint32_t lds[];
    uint2* SC = reinterpret_cast<uint2*>(lds);
    for (uint32_t i = threadIdx.x; i < a.nsearch * a.m; i += blockDim.x) SC[i] = a.table[i];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ltMask = (1ull << lane) - 1ull;
    constexpr TextShape kShape = textShape(SHAPE);
    LaneLds L;
    L.table = SC;
    L.slot = lds + a.tableWords;  // >= kTextTableMin: the window's block -1 stays in LDS
    L.winBlocks = SHAPE ? kShape.win : a.winBlocks;
    L.patBlocks = SHAPE ? kShape.pat : a.patBlocks;
    L.exactWindow = SHAPE ? kShape.exact : a.exactWindow != 0u;
    L.W = L.slot + threadIdx.x;
    L.P = L.slot + 3u * L.winBlocks * 256u + threadIdx.x;
    L.S = reinterpret_cast<uint2*>(L.slot + L.copyWords() * 256u) + threadIdx.x;
    const uint32_t winLen = L.winBlocks * 32u;
    const __amdgpu_buffer_rsrc_t textBuf = bufferOf(a.text3, a.text3Bytes);
    const __amdgpu_buffer_rsrc_t patBuf = bufferOf(a.pats3, a.pats3Bytes);
    const uint32_t m = a.m;
    // this launch's tasks: [tBase, taskCount) of the batch's list
    const uint32_t tEnd = min(*a.taskCount, a.taskCap);
    const uint32_t tBase = a.taskBegin ? min(*a.taskBegin, tEnd) : 0u;

    TextLane ln;
    bool exhausted = false, bad = false;
    TaskFeed feed(a.work, a.tasks + tBase, tEnd - tBase, a.sa, lane);
    HitWriter hits;
    __shared__ uint64_t waveClock[COUNT ? 8 : 1];  // count mode: the four waves' {born, drained}; else unused
    TextProbe<COUNT> probe(a, lane, waveClock);

    for (;;) {
        probe.iterBegin();
        // Starting a task costs a global round trip (window + pattern) that
        // stalls the whole wave, so idle lanes are refilled in batches: once
        // refillAt lanes are idle (or nothing else is left).
        const bool idle = !ln.have && ln.sp == 0 && !exhausted;
        const uint64_t idleMask = __ballot(idle);
        const bool busy = __any(ln.busy());
        const bool refill = !busy || __popcll(idleMask) >= a.refillAt;
        const bool need = refill && idle;
        uint64_t pending = refill ? idleMask : 0ull;
        if (pending) feed.resolveNext(lane);
        while (pending) {  // wave-uniform
            if (feed.chunkEmpty()) {
                if (!feed.haveNext) break;
                feed.advance(lane);
                if (feed.chunkEmpty()) continue;
            }
            uint4 t;
            const bool mine = feed.take(pending, lane, ltMask, t);
            if (mine && t.y != 0u) startTask(ln, t, L, m, textBuf, patBuf);  // |t| = 0: an unused reserved slot
            pending &= ~__ballot(mine);
        }
        if (feed.dry() && need && !ln.have) exhausted = true;
        if (a.stealAt && feed.dry()) probe.stolen(stealStage(ln, L, a.stealAt, lane, ltMask));
        if (!__any(ln.busy() || (!exhausted && !feed.dry()))) break;  // nothing left
        probe.refilled(feed.qDone, ln.busy(), refill);

        // ---- up to a.steps micro-steps per lane; a lane that reaches a leaf
        // holds it (stalls) until the emission below
        bool leaf = false;
        uint32_t leafStart = 0, leafE = 0;
        for (uint32_t step = 0; step < a.steps; ++step) {
            const bool pop = !ln.have && !leaf && ln.sp > 0;
            const TextNode top = L.stackGet(pop ? ln.sp - 1u : 0u);
            if (pop) { ln.cur = top; --ln.sp; ln.have = true; }
            const bool live = ln.have && !leaf;
            if (!__any(live)) break;  // wave-uniform

            const TextStepResult r = textStep<EDIT>(
                ln.cur, ln.sp, live, a.stackCap, m, winLen, [&](uint32_t p) { return L.row(ln.sBase + p); },
                [&](uint32_t o, bool fwd) { return chain32(L.P, o, fwd); },
                [&](uint32_t o, bool fwd) { return chain32(L.W, o, fwd); },
                [&](uint32_t d, const TextNode& n) { L.stackPut(d, n); });
            ln.cur = r.cur;
            ln.sp = r.sp;
            ln.have = live ? r.have : ln.have;
            if (r.leaf) { leaf = true; leafStart = r.leafStart; leafE = r.leafE; }
            bad = bad || r.bad;
            probe.stepped(r);
        }
        probe.stepsDone();
        hits.emit(a, leaf, lane, ltMask, ln.pid, ln.wb + leafStart, leafE);
        probe.emitted(feed.qDone);
    }
    probe.flush();
    hits.finish(a, lane);
    if (__any(bad) && lane == 0) atomicOr(a.flags, kFlagTextStack);
}

// The compiled variants, named once: the occupancy query and the launch take
// the same address.
const void* textBatchKernel(bool edit, bool count, int shape) {
#define SH_ROW(E, C) {(const void*)kSearchTextBatch<E, C, 0>, (const void*)kSearchTextBatch<E, C, 1>, \
                      (const void*)kSearchTextBatch<E, C, 2>}
    static const void* const kernels[2][2][kTextShapes] = {{SH_ROW(false, false), SH_ROW(false, true)},
                                                            {SH_ROW(true, false), SH_ROW(true, true)}};
#undef SH_ROW
    return kernels[edit][count][shape];
}

}  // namespace

// the compile-time shape matching a launch (0: the generic kernel)
int textShapeOf(uint32_t winBlocks, uint32_t patBlocks, bool exactWindow) {
    for (int shape = 1; shape < kTextShapes; ++shape) {
        const TextShape t = textShape(shape);
        if (winBlocks == t.win && patBlocks == t.pat && exactWindow == t.exact) return shape;
    }
    return 0;
}

int textBlocksPerCU(bool edit, bool count, int shape, size_t lds) {
    // (the variant that is launched: its registers differ by shape and count mode)
    int b = 0;
    SH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, textBatchKernel(edit, count, shape), 256, lds));
    return b;
}

void launchTextBatch(const TextBatchArgs& a, bool edit, bool count, uint32_t blocks, size_t lds, hipStream_t st) {
    const int shape = textShapeOf(a.winBlocks, a.patBlocks, a.exactWindow != 0u);
    void* args[] = {const_cast<TextBatchArgs*>(&a)};
    SH_HIP(hipLaunchKernel(textBatchKernel(edit, count, shape), dim3(blocks), dim3(256), args, lds, st));
}

}  // namespace sahara
