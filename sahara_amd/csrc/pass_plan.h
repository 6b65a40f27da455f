// pass_plan.h — what a pass decides before its first HIP call, as far as that
// needs no HIP: the knobs (every SAHARA_* variable of pass.cpp is read here,
// once at the start of each pass, so unsetting one restores its default), the
// batch boundaries and the FM / text geometry arithmetic. pass.cpp completes
// the plan with the occupancy queries. tests/pass_plan_check.cpp builds this
// header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <vector>

#include "fm_step.h"

namespace sahara {

// Text phase LDS: the scheme table comes first and takes at least one block of
// lane words (3 planes x 256 lanes), so that a read of a lane's window block -1
// (left reads near the window start) stays inside the workgroup's LDS.
constexpr uint32_t kTextTableMin = 3u * 256u;

// a list of pattern counts, ',' or ':' between them (zeros dropped)
inline std::vector<uint64_t> parseRamp(const char* e) {
    std::vector<uint64_t> v;
    for (const char* p = e; p && *p;) {
        char* end = nullptr;
        const unsigned long long x = std::strtoull(p, &end, 10);
        if (end == p) break;
        if (x) v.push_back(x);
        p = (*end == ',' || *end == ':') ? end + 1 : end;
    }
    return v;
}

struct PassKnobs {
    bool pipeline, dump, chunkSeeds, kmerPos, seedTasks;
    uint32_t fmLdsDepth, fmStealAt, stealAt, split, textSteps, refillAt, pollUs;
    uint32_t hitCap, taskCap;              // 0: unset
    unsigned long timerSlackNs;
    std::optional<long> batch, fmBpc, textBpc;
    std::vector<uint64_t> rampHead, rampTail;
};

inline PassKnobs readPassKnobs(bool verify) {
    auto num = [](const char* name) -> std::optional<long> {
        const char* e = std::getenv(name);
        return e ? std::optional<long>(std::atol(e)) : std::nullopt;
    };
    auto within = [](long lo, long v, long hi) { return std::max(lo, std::min(hi, v)); };
    PassKnobs k{};
    // SAHARA_PIPELINE=0 (profiling hook): batch after batch on one stream, so
    // that a kernel trace shows each kernel's stand-alone duration
    k.pipeline = num("SAHARA_PIPELINE").value_or(1) != 0;
    // (profiling hook) text geometry, the raw count-mode counters and, in
    // count mode, the first text launch's wave lives
    k.dump = std::getenv("SAHARA_DUMP_COUNTERS") != nullptr;
    // FM LDS: the scheme table, then the bottom fmLdsDepth DFS levels (16 B
    // per lane each; SAHARA_FM_LDS_DEPTH). None by default: with a depth-16
    // k-mer table the FM phase is light, its stack lives in L2, and its 1.2 KB
    // fit beside four text workgroups per CU (measured: depth 0 846M, 1 845M,
    // 4 817M reads/s at C3)
    // In the reference execution (verify off) every node is ranked from the
    // root, the DFS runs ~100x deeper trees and nothing else needs the LDS:
    // the bottom four levels there took C3 from 44.4M to 53.3M reads/s
    // (2: 49.9M, 8: 53.1M; profiles/r02_v1_sweep_ref_fm_lds_depth.txt).
    k.fmLdsDepth = (uint32_t)within(0, num("SAHARA_FM_LDS_DEPTH").value_or(verify ? 0 : 4), 8);
    // in-wave work stealing at the FM launch's end: in the reference execution
    // (verify off) the FM phase is the whole search and its tail idles half
    // the lanes (C5 2.7M -> 5.3M reads/s, C3 52.7M -> 62.7M); beside the
    // text phase it changed nothing measurable (C5 93.4M vs 94.8M, C3
    // within the spread; profiles/r04_fm_steal_ab.txt)
    k.fmStealAt = (uint32_t)within(0, num("SAHARA_FM_STEAL_AT").value_or(verify ? 0 : 8), 64);
    // text phase: in-wave work stealing while no task is in hand, once
    // SAHARA_STEAL_AT lanes of a wave are idle (0: off). Measured in one
    // process, alternating: C5 80.4M (off) -> 124.3M (1) / 129.5M (8) reads/s,
    // lanes busy 0.656 -> 0.890; C3 948M -> 1045M / 1056M, 0.787 -> 0.900
    k.stealAt = (uint32_t)within(0, num("SAHARA_STEAL_AT").value_or(8), 64);
    // intervals of <= split rows become text tasks (0: FM only)
    k.split = (uint32_t)std::max(0L, num("SAHARA_SPLIT").value_or(1));
    // Text-phase scheduling: micro-steps per lane per wave iteration, and the
    // idle lanes that trigger a batch refill. Two micro-steps per iteration
    // beat four by 5% on C3 and 2% on C5, C2 within noise
    // (profiles/r05_text_steps_ab.txt).
    k.textSteps = (uint32_t)std::max(1L, num("SAHARA_TEXT_STEPS").value_or(2));
    k.refillAt = (uint32_t)within(1, num("SAHARA_REFILL_AT").value_or(8), 64);
    // SAHARA_CHUNK_SEEDS=0: one seed launch per batch (pass.cpp makePlan)
    k.chunkSeeds = num("SAHARA_CHUNK_SEEDS").value_or(1) != 0;
    k.kmerPos = num("SAHARA_KMER_POS").value_or(1) != 0;      // (A/B) 0: k-mer seeds' tasks carry SA rows
    k.seedTasks = num("SAHARA_SEED_TASKS").value_or(1) != 0;  // 0: every seed goes through the FM kernel
    // The finisher's waits in a streamed call. A blocking-sync wait sleeps in
    // the driver until an interrupt wakes it, which took up to ~0.4 ms here (C2:
    // the row total after a 50 us scan waited 0.07 ms in one call, 0.37 ms in the
    // next); polling the event every pollUs microseconds keeps the thread asleep
    // almost all the time and wakes within one period. pollUs 0: blocking sync.
    k.pollUs = (uint32_t)std::max(0L, num("SAHARA_POLL_US").value_or(20));
    // the finisher's timer slack (0: the process default): its polls sleep 20 us;
    // Linux stretches a sleep by the thread's timer slack (50 us by default),
    // which a lone batch's locate chain waited for twice (C2: ~70 us per wait)
    k.timerSlackNs = (unsigned long)std::max(0L, num("SAHARA_TIMER_SLACK_NS").value_or(1000));
    // the hit and task buffers' first sizes (tests force overflow re-runs)
    if (auto v = num("SAHARA_HITCAP")) k.hitCap = (uint32_t)std::max(1L, *v);
    if (auto v = num("SAHARA_TASKCAP")) k.taskCap = (uint32_t)std::max(1L, *v);
    k.batch = num("SAHARA_BATCH");        // maxBatchOf
    k.fmBpc = num("SAHARA_FM_BPC");       // workgroups per CU (pass.cpp makePlan)
    k.textBpc = num("SAHARA_TEXT_BPC");
    k.rampHead = parseRamp(std::getenv("SAHARA_RAMP"));  // batchStarts
    k.rampTail = parseRamp(std::getenv("SAHARA_RAMP_END"));
    return k;
}

// patterns per batch: 4M (2M in a streamed call: its first batch waits
// for the host to pack and upload it, its last one's hits for the
// download, so smaller ones shorten both ends; C3 compact reads path
// 584-615M -> 668-689M reads/s, profiles/r03_pcie_batch_sweep.txt),
// fewer for schemes with many searches (work items must fit 2^31);
// SAHARA_BATCH (`batch`) sets it (tests of the pipeline). granularity g > 1
// (the pair stage: 4, a pair's qids stay in one batch): rounded down to a
// multiple of g, and g where that leaves nothing (one group per batch).
inline uint64_t maxBatchOf(std::optional<long> batch, bool streaming, uint32_t nsearch, bool compactRecs,
                           uint64_t granularity = 1) {
    const uint64_t most = (1ull << 31) / nsearch;
    uint64_t mb = std::min<uint64_t>(streaming ? 1ull << 21 : 1ull << 22, most);
    if (batch) mb = std::max<uint64_t>(1, std::min<uint64_t>(most, (uint64_t)*batch));
    if (compactRecs) mb = std::min<uint64_t>(mb, 1ull << 27);  // compact records: qid - q0 < 2^28
    return granularity > 1 ? std::max<uint64_t>(granularity, mb / granularity * granularity) : mb;
}

// a hit or task buffer's first size for batches of maxBatch patterns; a pass
// grows them on overflow
inline uint32_t firstWorkCap(uint64_t maxBatch) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, 8 * maxBatch), 1u << 30);
}

// batch boundaries: equal batches of <= maxBatch patterns, or (pipelined,
// SAHARA_RAMP / SAHARA_RAMP_END: lists of pattern counts) given first and
// last batches around equal middle ones. granularity g > 1 (npat a multiple
// of g, maxBatch one from maxBatchOf): the same plan made in groups of g
// patterns, a ramp entry below g taken as one group and any other rounded
// down to whole groups, so every boundary is a multiple of g, no batch is
// empty and none exceeds maxBatch.
inline std::vector<uint64_t> batchStarts(uint64_t npat, uint64_t maxBatch, std::vector<uint64_t> head,
                                         std::vector<uint64_t> tail, bool serial, uint64_t granularity = 1) {
    if (granularity > 1) {
        const uint64_t g = granularity;
        for (auto* ramp : {&head, &tail})
            for (auto& x : *ramp) x = std::max<uint64_t>(1, x / g);
        std::vector<uint64_t> groups = batchStarts(npat / g, std::max<uint64_t>(1, maxBatch / g), head, tail, serial);
        for (auto& x : groups) x *= g;
        return groups;
    }
    std::vector<uint64_t> bstart{0};
    uint64_t edges = 0;
    for (auto& x : head) edges += x = std::min(x, maxBatch);
    for (auto& x : tail) edges += x = std::min(x, maxBatch);
    if (serial || npat < edges + maxBatch) head.clear(), tail.clear(), edges = 0;
    for (uint64_t x : head) bstart.push_back(bstart.back() + x);
    const uint64_t mid = npat - edges, q0 = bstart.back(), nmid = (mid + maxBatch - 1) / maxBatch;
    for (uint64_t i = 1; i <= nmid; ++i) bstart.push_back(q0 + mid * i / nmid);
    for (uint64_t x : tail) bstart.push_back(bstart.back() + x);
    return bstart;
}

// FM phase: LDS bytes (the scheme table, then ldsDepth DFS levels of 16 B per
// lane); the entries a lane's DFS stack can hold: fmStackCap (fm_step.h)
inline size_t fmLdsBytes(uint32_t nsearch, uint32_t m, uint32_t ldsDepth) {
    return (size_t)((nsearch * m + 3u) & ~3u) * 4 + (size_t)ldsDepth * 256 * 16;
}

// text phase geometry (LDS per lane: window | pattern | stack)
// window: |t| + what both sides can still consume <= m + 2k symbols, plus
// the block alignment of its start (31 symbols); 3 words per block
// (exact start: m + 2k symbols in whole blocks, copied funnel-shifted from
// one block more, where both fit the copy's 8 loads; else the block-aligned
// start below it)
struct TextGeometry {
    bool exactWindow;
    uint32_t winBlocks, textStack, tableWords;
    size_t lds;
};
inline TextGeometry textGeometry(uint32_t m, uint32_t maxErr, uint32_t patBlocks, uint32_t nsearch) {
    TextGeometry g{};
    const uint32_t exactBlocks = (m + 2 * maxErr + 31) / 32;
    g.exactWindow = exactBlocks + 1 <= 8 && patBlocks <= 8;
    g.winBlocks = g.exactWindow ? exactBlocks : (m + 2 * maxErr + 31 + 31) / 32;
    g.textStack = 2 * maxErr + 2;
    g.tableWords = std::max<uint32_t>(2 * nsearch * m, kTextTableMin);
    g.lds = (size_t)g.tableWords * 4 + (size_t)256 * (3 * (g.winBlocks + patBlocks) + 2 * g.textStack) * 4;
    return g;
}

// The one geometry of a pass of several rounds: every round runs with the
// FM LDS and stack, the text geometry and the batch size of the worst round,
// i.e. of the most searches and the most errors of any round (a round with
// fewer of either uses a prefix of the tables' LDS, a shorter stack and a
// window that is wider than it needs).
struct WorstRound {
    uint32_t nsearch = 0, maxErr = 0;
};
template <typename Rounds>
inline WorstRound worstRound(const Rounds& rounds) {
    WorstRound w;
    for (const auto& r : rounds) {
        w.nsearch = std::max(w.nsearch, r.nsearch);
        w.maxErr = std::max(w.maxErr, r.maxErr);
    }
    return w;
}

// The stages that a batch's sorted whole hits go through before they leave
// the device, in the order they run (pass.cpp Pass::stages): loci (loci.hip),
// the mate rescue (rescue.hip), pairs (pairs.hip), --max_hits (hits.hip
// limitBatch). The rescue looks in the pair rule's window: it counts as on
// only with pairs on.
enum Stage : uint32_t { kStageLoci, kStageRescue, kStagePairs, kStageLimit, kStages };
struct StagesOn {
    bool on[kStages];
};
inline StagesOn stagesOn(bool loci, bool pairs, bool rescue, bool limit) {
    return {{loci, rescue && pairs, pairs, limit}};
}
// The segments rule. When a stage starts, the batch's per-query segments
// (qoff) describe the records it is given: the sort leaves them so, and a
// stage that changed the records (loci or pairs dropped some, the rescue
// added some) writes them again iff a later stage runs on the batch, which is
// what this says (search.h BatchView::later, hits.hip replaceBatch). Every
// stage after the first reads them.
inline bool laterStage(const StagesOn& s, uint32_t stage) {
    for (uint32_t i = stage + 1; i < kStages; ++i)
        if (s.on[i]) return true;
    return false;
}

// Everything a pass fixes before its first HIP call (pass.cpp makePlan);
// the stages read it and nothing else decides
struct PassPlan {
    PassKnobs k;
    bool count = false, serial = false;
    uint64_t maxBatch = 0;
    std::vector<uint64_t> bstart;          // batch b: patterns [bstart[b], bstart[b + 1])
    size_t fmLds = 0;                      // FM phase: LDS bytes, grids (the first batch's), DFS stack
    uint32_t blocks = 0, firstBlocks = 0, stackCap = 0, stackLevels = 0;
    TextGeometry tx{};                     // text phase: geometry, kernel shape, workgroups per CU, grid
    int textShape = 0, textBpc = 0;
    uint32_t textBlocks = 0;
    uint32_t split = 0, toText = 0;        // k.split, 0 when the text phase cannot run; single-row seeds are tasks
    // the first batch's text phase starts on its seed tasks (early), seeded
    // chunk by chunk as the upload arrives (chunked0); the finisher sleeps in
    // its waits; (count mode, k.dump) the first text launch's wave lives
    bool early = false, chunked0 = false, sleepy = false, probe = false;
    // rounds per batch (besthits: one per exact-j scheme, else 1). The
    // geometry above is planned once, for the worst round: the most searches,
    // the most errors, the largest tables (worstRound).
    uint32_t rounds = 1;
    uint64_t nbatch() const { return bstart.size() - 1; }
};

}  // namespace sahara
