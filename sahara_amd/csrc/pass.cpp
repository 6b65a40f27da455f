// pass.cpp — one pass of the search over the staged patterns: batches
// through seeds, FM phase, text phase, locate, sort and decode on the
// context's streams, then through the stages that are on
// (loci, mate rescue, pairs, --max_hits: one driver, Pass::stages, over one
// view of the batch) into the call's sink; and the pass
// over every part of a multi-part index.
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <thread>

#include <sys/prctl.h>

#include "ctx.h"
#include "align_core.h"
#include "best_pairs_core.h"
#include "rescue_core.h"

namespace sahara {

DeviceIndex& partOf(Ctx* c, uint32_t p) { return p == 0 ? c->I : c->more.at(p - 1); }

// Search over a multi-part index: the pass runs over every part in turn (the
// staged patterns and scheme are shared; every part has the same k-mer
// depth), its hits get the part's record offset, and one stable sort by qid
// restores the canonical (qid, seq_id, pos, err) order, since part p's
// records all follow part p - 1's. Exact under P-strict: a DFS node exists in
// the whole index iff its interval is non-empty in some part, and its rows
// are the union of its rows over the parts. Hits reach the
// host after the last part (no per-batch sink).
// Loci on a multi-part index: the stage runs per part, inside each part's
// pass (Pass::finish), on the part's own record ids. A locus lies within one
// record and a record lies wholly in one part, so the loci of the merged hits
// are the union of the parts' loci, each with the same records in the same
// order: filtering per part equals filtering after the merge, and the merge
// moves a tenth of the records.
// Pairs on a multi-part index: per part in the same way. Two concordant hits
// lie on one record and a record lies wholly in one part, so a hit has a mate
// among the merged hits iff it has one among its own part's: the union of the
// parts' kept hits is the kept hits of the merged call. (A pair may keep hits
// in several parts: the stats' pairs then count it once per part.)
// The mate rescue on a multi-part index: per part as well. A window lies on
// the anchor's record and a record lies wholly in one part, whose text and
// record starts the scan reads; an anchor of the merged hits is an anchor of
// its part's hits, since its mates could only lie on its own record.
// Best pairs on a multi-part index: refused. A pair's best total is a minimum
// over all its placements, and the cut per part would keep in each part what
// is best there, not what is best over all parts.
void checkPairsCall(const Ctx* c, uint64_t npat, uint32_t len) {
    if (c->rescue.on) {  // (docs/semantics.md "Mate rescue", refused calls)
        if (!c->pairs.on) throw Error("rescue: needs pairs on (a mate is looked for in the pair rule's fragment window)");
        if (len > kAlignMaxLen)
            throw Error("rescue: the pattern length " + std::to_string(len) + " is above " + std::to_string(kAlignMaxLen));
        if (c->pairs.maxFrag >= len) {
            const PairDist d = pairDist(len, c->pairs.minFrag, c->pairs.maxFrag);
            if (d.dmax - d.dmin >= kRescueMaxWindow)
                throw Error("rescue: the fragment window of " + std::to_string(d.dmax - d.dmin + 1) +
                            " starts is above SAHARA_RESCUE_MAX_WINDOW (" + std::to_string(kRescueMaxWindow) + ")");
        }
    }
    if (c->pairs.links && !c->pairs.best)  // (docs/semantics.md "Pair links", refused calls)
        throw Error("pair links: needs best pairs on (a link is a record of the best-pairs rule)");
    if (c->pairs.best) {  // (docs/semantics.md "Best pairs", refused calls)
        if (!c->pairs.on) throw Error("best pairs: needs pairs on (the placements ranked are the pair rule's)");
        if (!c->more.empty())
            throw Error("best pairs: a multi-part index is not supported (a pair's best total over one part is not "
                        "its best over all parts)");
    }
    if (!c->pairs.on) return;
    if (c->pairs.maxFrag < len)
        throw Error("pairs: max_fragment " + std::to_string(c->pairs.maxFrag) + " is below the pattern length " +
                    std::to_string(len));
    if (npat % 4)
        throw Error("pairs: " + std::to_string(npat) + " patterns are no multiple of 4 (a pair is two mates and "
                    "their reverse complements)");
}

void run(Ctx* c, bool count) {
    c->stageStats = Ctx::StageStats{};  // of this call: the passes below add to them
    if (c->sk.staged) checkPairsCall(c, c->npat, c->m);
    // best pairs: the call's pair summaries, one per four patterns (runPass fills them with "keeps nothing",
    // the batches' pair stages write over that); a call with the mode off leaves none behind
    c->pairs.summaryOn = c->sk.staged && c->pairs.on && c->pairs.best;
    c->pairs.summaryPairs = c->pairs.summaryOn ? c->npat / 4 : 0;
    if (c->pairs.summaryOn) c->pairs.summary.reserve(std::max<uint64_t>(c->pairs.summaryPairs, 1));
    // pair links: one per hit of the call, written per batch from c->nout on; --max_hits would cut linked hits
    if (c->sk.staged && c->pairs.links && c->sk.limitN)
        throw Error("pair links: a call with max_hits is not supported (the cut would drop linked hits)");
    c->pairs.linksOn = c->pairs.summaryOn && c->pairs.links;
    c->pairs.linkCount = 0;
    if (c->more.empty()) return runOne(c, count);
    // (rounds mask a query by its rows in one part; "found" is decided across the parts: capi.cpp bestOnHost)
    if (c->rounds.size() > 1) throw Error("a pass of several rounds needs a single-part index");
    const ScopeExit routeBack([c, route = c->sk.route] { c->sk.route = route; });
    c->sk.route = HitRoute::Device;
    sahara_stats T{};
    uint64_t total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t p = 0; p <= c->more.size(); ++p) {
        if (p) std::swap(c->I, c->more[p - 1]);
        {
            const ScopeExit partBack([c, p] {
                if (p) std::swap(c->I, c->more[p - 1]);
            });
            runOne(c, count);
        }
        if (c->outAll.cap < total + c->nout)  // grow, keeping the parts so far
            c->outAll.growKeeping(std::max<uint64_t>((total + c->nout) + (total + c->nout) / 4, 1024), total, c->st);
        launchOffsetSeq(c->out.ptr, c->nout, c->partRec0[p], c->outAll.ptr + total, c->st);
        total += c->nout;
        const sahara_stats& S = c->stats;  // the parts' work adds up
        T.patterns = S.patterns;
        T.search_grid = S.search_grid;
        T.text_grid = S.text_grid;
        T.pipelined = S.pipelined;
        T.best_rounds = S.best_rounds;
        for (uint64_t sahara_stats::*f :
             {&sahara_stats::batches, &sahara_stats::cursors, &sahara_stats::nodes, &sahara_stats::rank_nodes,
              &sahara_stats::ext_lines, &sahara_stats::lf_steps, &sahara_stats::text_nodes,
              &sahara_stats::conversions, &sahara_stats::fm_iterations, &sahara_stats::text_iterations,
              &sahara_stats::text_active, &sahara_stats::text_refills, &sahara_stats::text_cycles_refill,
              &sahara_stats::text_cycles_step, &sahara_stats::text_cycles_emit, &sahara_stats::text_compare_steps,
              &sahara_stats::text_steps, &sahara_stats::text_launches,
              &sahara_stats::text_pos_tasks, &sahara_stats::text_stolen, &sahara_stats::best_skipped})
            T.*f += S.*f;
        for (double sahara_stats::*f : {&sahara_stats::search_ms, &sahara_stats::locate_ms, &sahara_stats::sort_ms,
                                        &sahara_stats::text_ms, &sahara_stats::seed_ms})
            T.*f += S.*f;
        T.search_launches += S.search_launches;
    }
    if (c->out.cap < total) {
        c->out.release();
        c->out.reserve(std::max<uint64_t>(total, 1024));
    }
    sortHitsByQid(c->outAll.ptr, total, c->npat, c->out.ptr, c->merge, c->tmp, c->st);
    SH_HIP(hipStreamSynchronize(c->st));
    c->sk.done = 0;
    c->nout = total;
    T.hits = total;
    T.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    T.stage_ms = c->stageMs;
    for (int b = 0; b < 3; ++b) T.upload_chunks[b] = c->stats.upload_chunks[b];
    c->stats = T;
}

void runOne(Ctx* c, bool count) {
    if (!c->sk.staged) throw Error("sahara_gpu_run: nothing staged");
    auto t0 = std::chrono::steady_clock::now();
    sahara_stats S{};
    bool overflow = false;
    const Ctx::StageStats stagesBefore = c->stageStats;  // (a multi-part call's earlier parts)
    runPass(c, count, false, S, overflow);
    if (overflow) {
        S = sahara_stats{};
        c->stageStats = stagesBefore;  // the batches finished before the overflow are redone
        runPass(c, count, true, S, overflow);
    }
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    S.stage_ms = c->stageMs;
    c->stats = S;
    if (c->pairs.linksOn) c->pairs.linkCount = c->nout;  // (one part: the pass's hits are the call's)
}

const sahara_hit* Ctx::wholeHits() {
    if (outStale) {  // (the pass is over: its streams are synchronised)
        if (out.cap < nout) out.growKeeping(nout, out.cap, st);  // other batches' hits are in it already
        uint64_t b0 = 0;
        for (size_t b = 0; b < batchEnd.size(); b0 = batchEnd[b], ++b)
            if (batchDirect[b])
                launchExpandRecs(outRecs.ptr + b0, batchEnd[b] - b0, batchQ0[b], I.dRecStarts.ptr,
                                 (uint32_t)I.recStarts.size(), out.ptr + b0, st);
        SH_HIP(hipStreamSynchronize(st));
        outStale = false;
    }
    return out.ptr;
}

void initWorkCaps(Ctx* c, uint64_t maxBatch, const PassKnobs& k) {
    if (c->hitCap == 0) c->hitCap = k.hitCap ? k.hitCap : firstWorkCap(maxBatch);
    if (c->taskCap == 0) c->taskCap = k.taskCap ? k.taskCap : firstWorkCap(maxBatch);
}

void reserveSlot(Ctx* c, Ctx::Slot& sl) {
    sl.hits.reserve((size_t)c->hitCap + 1);
    sl.rank.reserve((size_t)c->hitCap + 1);
    sl.tasks.reserve((size_t)c->taskCap);
}

// the locate chain's per-batch buffers and the first nslots slots' per-query row counts
void reserveLocate(Ctx* c, uint64_t maxBatch, uint64_t nslots) {
    c->qoff.reserve(maxBatch + 1);
    c->big.reserve(maxBatch);
    c->huge.reserve(maxBatch);
    for (uint64_t i = 0; i < nslots; ++i) c->slot[i].qcnt.reserve(maxBatch + 1);
}

void growCap(uint32_t& cap, uint32_t seen) {
    const uint64_t want = (uint64_t)seen + seen / 4 + 1024;
    if (want >= (1ull << 32) - 2) throw Error("a work buffer would exceed 2^32 entries in one batch");
    cap = std::max<uint32_t>(cap, (uint32_t)want);
}

// The finisher's waits in a streamed call poll the event every pollUs
// microseconds (pass_plan.h SAHARA_POLL_US); pollUs 0: blocking sync.
static void waitSleepy(hipEvent_t e, uint32_t pollUs) {
    if (!pollUs) {
        SH_HIP(hipEventSynchronize(e));
        return;
    }
    for (;;) {
        const hipError_t r = hipEventQuery(e);
        if (r == hipSuccess) return;
        if (r != hipErrorNotReady) SH_HIP(r);
        std::this_thread::sleep_for(std::chrono::microseconds(pollUs));
    }
}

// The plan of one pass: the knobs and the HIP-free arithmetic of pass_plan.h,
// completed by the occupancy queries. `redo`: the serial re-run after an
// overflow (SAHARA_PIPELINE=0 makes every pass serial).
static PassPlan makePlan(Ctx* c, bool count, bool redo) {
    PassPlan P;
    P.k = readPassKnobs(c->verify);
    const PassKnobs& k = P.k;
    const bool serial = P.serial = redo || !k.pipeline;
    P.count = count;
    P.rounds = (uint32_t)c->rounds.size();
    // (c->nsearch, c->maxErr: the worst round's, what stageSchemes left there)
    const WorstRound worst = worstRound(c->rounds);
    if (worst.nsearch != c->nsearch || worst.maxErr != c->maxErr) throw Error("staged rounds do not match their plan");
    const uint32_t sigma = c->I.sigma;
    P.fmLds = fmLdsBytes(c->nsearch, c->m, k.fmLdsDepth);
    const int fullBpc = searchBlocksPerCU(sigma, c->edit, P.fmLds);
    int bpc = fullBpc;
    // Overlapped with the text phase of the previous batch, the FM phase
    // (memory-latency bound) runs one workgroup per CU beside three text
    // workgroups; alone it takes all that fit. (Measured at C3 with pruned
    // text steps: text 3 + FM 2 846-873M reads/s, text 4 + FM 1 845-847M;
    // after the atomic-free locate chain, text 3 + FM 1 917-957M against
    // text 3 + FM 2 883-905M and FM 3 847-890M, alternating runs on one box:
    // 115-131 VGPRs per FM wave leave the SIMDs' registers to the text waves
    // and the locate chain.)
    // (pairs: a pair's four qids stay in one batch, pairs.hip)
    const uint64_t granularity = c->pairs.on ? 4 : 1;
    P.maxBatch = maxBatchOf(k.batch, c->sk.streaming, c->nsearch, c->sk.route == HitRoute::Records, granularity);
    const uint64_t batchesHere = (c->npat + P.maxBatch - 1) / P.maxBatch;
    if (!serial && batchesHere > 1 && c->verify) bpc = 1;
    if (k.fmBpc) bpc = (int)std::max<long>(1, std::min<long>(fullBpc, *k.fmBpc));
    P.blocks = (uint32_t)(c->numCU * bpc);
    // the first batch's FM phase has nothing to overlap with: full occupancy
    P.firstBlocks = k.fmBpc ? P.blocks : (uint32_t)(c->numCU * fullBpc);
    // a ring of stackCap levels per lane (work stealing moves a stack's bottom up)
    P.stackLevels = P.stackCap = fmStackCap(c->maxErr, sigma);

    P.tx = textGeometry(c->m, c->maxErr, c->patBlocks, c->nsearch);
    // the text phase addresses text and a batch's patterns with 32-bit buffer offsets
    const bool textFits = text3Blocks(c->I.n) * 16 <= 0xFFFFFF00ull &&
                          P.maxBatch * c->patBlocks * 16 <= 0xFFFFFF00ull;
    P.textShape = textShapeOf(P.tx.winBlocks, c->patBlocks, P.tx.exactWindow);
    auto textAlone = [&] { return textBlocksPerCU(c->edit, count, P.textShape, P.tx.lds); };
    int tbpc = c->verify && c->m <= 2047 && P.tx.lds <= 160 * 1024 && textFits ? textAlone() : 0;
    // overlapped with the FM phase, three text workgroups per CU beside its one
    // (four would fit: r2 v8 measured text 4 against 3 in alternating pairs,
    // C3 914-943M vs 880-952M on one box and 873-914M vs 953-956M on another,
    // C2 950-1013M vs 956-1026M: the sign flips with the box)
    if (!serial && batchesHere > 1) tbpc = std::min(tbpc, 3);
    if (k.textBpc && tbpc > 0) tbpc = (int)std::max<long>(1, std::min<long>(textAlone(), *k.textBpc));
    if (k.dump)
        std::fprintf(stderr, "text geometry: shape %d lds %zu blocks/CU %d (alone %d) serial %d\n", P.textShape, P.tx.lds,
                     tbpc, textAlone(), (int)serial);
    P.textBpc = tbpc;
    P.textBlocks = (uint32_t)(c->numCU * std::max(tbpc, 1));
    P.split = tbpc > 0 ? k.split : 0u;
    P.toText = P.split >= 1 && k.seedTasks ? 1u : 0u;
    // (pipelined) the first batch's text phase starts on its seed tasks while
    // its FM phase runs; a device-resident lone batch does not: its FM phase
    // runs at full occupancy, and its text phase split in two measured 45M
    // against 68M reads/s at C5 (r1)
    // A streamed call seeds its first batch in two parts, the first chunk's
    // as soon as that chunk is up, and starts the text phase on their tasks
    // while the rest of the batch uploads, seeds and runs its FM phase, also
    // when the call is one batch (C5 95.2M -> 100.2M, C2 500M -> 503M, C3
    // 792M -> 805M; without the split seeds a lone batch's early text phase
    // lost: C5 89.9M, C2 475M; profiles/r04_chunk_seeds_ab.txt).
    const bool chunkSeeds = c->sk.streaming && !serial && P.split && k.chunkSeeds;
    // (several rounds: no early text launch, the first batch's rounds run like every other's)
    P.early = !serial && P.split && (batchesHere > 1 || chunkSeeds) && P.rounds == 1;
    P.chunked0 = P.early && chunkSeeds;
    // a streamed call's finisher sleeps in its waits while the calling thread
    // and the pool pack (device-resident runs spin)
    P.sleepy = c->sk.streaming && !serial;
    P.probe = count && k.dump;
    P.bstart = batchStarts(c->npat, P.maxBatch, k.rampHead, k.rampTail, serial, granularity);
    return P;
}

static SearchArgs searchArgs(Ctx* c, const PassPlan& P, Ctx::Slot& sl, uint64_t b, uint32_t r) {
    const uint64_t q0 = P.bstart[b];
    const Ctx::Round& R = c->rounds[r];
    SearchArgs a{};
    a.occF = c->I.occF.ptr;
    a.occR = c->I.occR.ptr;
    for (int i = 0; i < 8; ++i) a.C[i] = (uint32_t)c->I.C[i];
    a.n = (uint32_t)c->I.n;
    a.pats = c->pats.ptr + q0 * c->patWords;
    a.patWords = c->patWords;
    a.m = c->m;
    a.nsearch = R.nsearch;
    a.nitems = (uint32_t)((P.bstart[b + 1] - q0) * R.nsearch);
    a.seeds = sl.seeds.ptr;
    a.seedItem = sl.seedItem.ptr;
    a.seedCount = sl.small.ptr + kSwSeedCount;
    a.scheme = c->scheme.ptr + R.schemeAt;
    a.work = sl.queues.ptr + kQueueSeeds;
    a.hitCount = sl.small.ptr + kSwHitCount;
    a.flags = sl.small.ptr + kSwFlags;
    a.filled = sl.small.ptr + kSwFilled;
    a.taskCount = sl.small.ptr + kSwTaskCount;
    a.stack = c->stack.ptr;
    a.stackCap = P.stackCap;
    a.stackLevels = P.stackLevels;
    a.stealAt = P.k.fmStealAt;
    a.hits = sl.hits.ptr;
    a.hitCap = c->hitCap;
    a.counters = c->counters.ptr;
    a.tasks = sl.tasks.ptr;
    a.taskCap = c->taskCap;
    a.split = P.split;
    a.ldsDepth = P.k.fmLdsDepth;
    a.qcnt = sl.qcnt.ptr;
    a.rank = sl.rank.ptr;
    return a;
}

// starting cursors; reference execution (verify off) ranks every node
// from the root, so it does not use the k-mer table
static SeedArgs seedArgs(Ctx* c, const PassPlan& P, Ctx::Slot& sl, uint64_t b, uint32_t r) {
    const Ctx::Round& R = c->rounds[r];
    SeedArgs sd{};
    sd.pats = c->pats.ptr + P.bstart[b] * c->patWords;
    sd.patWords = c->patWords;
    sd.nsearch = R.nsearch;
    sd.nitems = (uint32_t)((P.bstart[b + 1] - P.bstart[b]) * R.nsearch);
    sd.n = (uint32_t)c->I.n;
    sd.kmer = c->verify && c->I.kmerK ? c->I.kmer.ptr : nullptr;
    sd.kmerK = c->I.kmerK;
    sd.kmerPos = c->I.kmerPos && P.k.kmerPos ? 1u : 0u;
    sd.kmerStart = c->kmerStart.ptr + R.kmerAt;
    sd.seeds = sl.seeds.ptr;
    sd.seedItem = sl.seedItem.ptr;
    sd.seedCount = sl.small.ptr + kSwSeedCount;
    sd.m = c->m;
    sd.toText = P.toText;
    sd.tasks = sl.tasks.ptr;
    sd.taskCap = c->taskCap;
    sd.taskCount = sl.small.ptr + kSwTaskCount;
    sd.flags = sl.small.ptr + kSwFlags;
    sd.counters = P.count ? c->counters.ptr : nullptr;
    // a later round seeds only the patterns without a row so far (issueFM)
    sd.skip = r ? sl.qcnt.ptr : nullptr;
    return sd;
}

// the launch over all of the batch's tasks (an early first batch's two
// launches change taskBegin, taskCount and work: issueText)
static TextBatchArgs textArgs(Ctx* c, const PassPlan& P, Ctx::Slot& sl, uint64_t b, uint32_t r) {
    const uint64_t q0 = P.bstart[b];
    const Ctx::Round& R = c->rounds[r];
    TextBatchArgs t{};
    t.sa = c->I.saFull.ptr;
    t.text3 = c->I.text3.ptr;
    t.pats3 = c->pats3.ptr + q0 * c->patBlocks;
    t.patBlocks = c->patBlocks;
    t.text3Bytes = (uint32_t)std::min<uint64_t>(text3Blocks(c->I.n) * 16, 0xFFFFFF00ull);
    t.pats3Bytes = (uint32_t)std::min<uint64_t>((P.bstart[b + 1] - q0) * c->patBlocks * 16, 0xFFFFFF00ull);
    t.m = c->m;
    t.nsearch = R.nsearch;
    t.table = reinterpret_cast<const uint2*>(c->cover.ptr + R.coverAt);
    t.tasks = sl.tasks.ptr;
    t.taskCount = sl.small.ptr + kSwTaskCount;
    // a later round's tasks follow the earlier rounds' in the slot's list
    // (search indices of its own table): from kRoundReset's snapshot on
    t.taskBegin = r ? sl.small.ptr + kSwRoundTasks : nullptr;
    t.taskCap = c->taskCap;
    t.work = sl.queues.ptr + kQueueSeedTasks;
    t.hits = sl.hits.ptr;
    t.hitCap = c->hitCap;
    t.hitCount = sl.small.ptr + kSwHitCount;
    t.filled = sl.small.ptr + kSwFilled;
    t.flags = sl.small.ptr + kSwFlags;
    t.counters = c->counters.ptr;
    t.winBlocks = P.tx.winBlocks;
    t.exactWindow = P.tx.exactWindow ? 1u : 0u;
    t.stackCap = P.tx.textStack;
    t.tableWords = P.tx.tableWords;
    t.steps = P.k.textSteps;
    t.refillAt = P.k.refillAt;
    t.stealAt = P.k.stealAt;
    t.qcnt = sl.qcnt.ptr;
    t.rank = sl.rank.ptr;
    t.probe = P.probe ? 1u : 0u;
    t.isFirst = b == 0 && r == 0 ? 1u : 0u;
    return t;
}

// words of Ctx::small in a batch's locate chain: its flags, its long and huge segment counts
enum : uint32_t { kLocFlags = 2, kLocSegCounts = 4 };

static LocateArgs locateArgs(Ctx* c, Ctx::Slot& sl, uint64_t nhits) {
    LocateArgs la{};
    la.hits = sl.hits.ptr;
    la.nhits = nhits;
    la.qoff = c->qoff.ptr;
    la.rank = sl.rank.ptr;
    la.occF = c->I.occF.ptr;
    for (int i = 0; i < 8; ++i) la.C[i] = (uint32_t)c->I.C[i];
    la.samples = c->I.samples.ptr;
    la.rate = c->I.rate;
    la.keys = c->k0.ptr;
    la.flags = c->small.ptr + kLocFlags;
    la.counters = c->counters.ptr + kCtLfSteps;
    la.sa = c->I.saFull.ptr;
    la.useSA = c->locateSA ? 1u : 0u;
    return la;
}

// One pass in flight: the context, the plan, and the little that its stages
// change. The issuing thread runs issueFM(b) and issueText(b); the finisher
// thread runs finish(b) and, one batch later, finishCheck(b).
struct Pass {
    Ctx* c;
    const PassPlan& P;
    sahara_stats& S;
    bool& overflow;
    hipStream_t sA, sB, sC, sD;          // FM phase; text; locate / sort; seeds (serial: all Ctx::st)
    uint32_t seenTask = 0, seenHit = 0;  // pipelined overflow: the caps the re-run needs
    bool stageRan[kStages] = {};         // by Stage: the batch just finished ran it (finishCheck reads its span)

    Ctx::Slot& slotOf(uint64_t b) const { return c->slot[b % Ctx::kSlots]; }

    // a slot's counters and queues are zero when its `free` event fires:
    // at the pass's start for the first use (resetSlot), after its locate
    // for the next (finish: kBatchTotals has cleared them, freeSlot)
    void resetSlot(Ctx::Slot& sl, hipStream_t s) {
        SH_HIP(hipMemsetAsync(sl.small.ptr, 0, kSlotWords * sizeof(uint32_t), s));
        SH_HIP(hipMemsetAsync(sl.queues.ptr, 0, kQueuesWords * sizeof(uint32_t), s));
        SH_HIP(hipEventRecord(sl.free, s));
    }
    void freeSlot(Ctx::Slot& sl, hipStream_t s) { SH_HIP(hipEventRecord(sl.free, s)); }

    // the batch's seed tasks are all written (stream sD): the first batch's
    // text phase launches on them (the count snapshot in kSwSeedTasks) before
    // its FM phase ends
    void seedTasksDone(Ctx::Slot& sl) {
        SH_HIP(hipMemcpyAsync(sl.small.ptr + kSwSeedTasks, sl.small.ptr + kSwTaskCount, 4, hipMemcpyDeviceToDevice, sD));
    }

    // The events round r of the slot's batch records: the slot's own for the
    // last round (finish waits for its textDone), sl.earlier[r] before it.
    struct RoundEv {
        hipEvent_t fmStart, seedDone, fmBegin, fmDone, textStart, textDone;
    };
    RoundEv eventsOf(Ctx::Slot& sl, uint32_t r) const {
        if (r + 1 == P.rounds) return {sl.fmStart, sl.seedDone, sl.fmBegin, sl.fmDone, sl.textStart, sl.textDone};
        Ctx::Slot::RoundEvents& e = sl.earlier[r];
        return {e.fmStart, e.seedDone, e.fmBegin, e.fmDone, e.textStart, e.textDone};
    }

    // Round r of batch b: its seeds (sD) and FM phase (sA); issueText(b, r)
    // follows. The event chain of a batch of several rounds, all in its slot:
    //   free -> [sD] seeds(0) -> [sA] FM(0) -> [sB] text(0) -> textDone(0)
    //        -> [sD] round reset, seeds(1, skip = qcnt) -> [sA] FM(1) -> [sB] text(1) -> textDone(1) -> ...
    //        -> textDone(last) -> [sC] finish.
    // Round r's seeds wait for round r - 1's textDone: they read the slot's
    // per-query row counts as their mask, which the FM and text kernels of
    // round r - 1 add to until then; nothing writes them while the seeds run,
    // as round r's FM phase waits for the seeds. (Without that wait a query
    // found late in round r - 1 would be searched again: silently wrong hits.)
    // The reset of the seed count and the queue words sits behind the same
    // wait, so no kernel of round r - 1 still reads them.
    void issueFM(uint64_t b, uint32_t r) {
        Ctx::Slot& sl = slotOf(b);
        const std::vector<uint64_t>& bstart = P.bstart;
        const RoundEv ev = eventsOf(sl, r);
        const uint32_t nitems = (uint32_t)((bstart[b + 1] - bstart[b]) * c->rounds[r].nsearch);
        if (r == 0) {
            reserveSlot(c, sl);
            SH_HIP(hipStreamWaitEvent(sA, sl.free, 0));  // the slot's previous batch is fully consumed
            const uint32_t most = (uint32_t)((bstart[b + 1] - bstart[b]) * c->nsearch);  // of any round
            sl.seeds.reserve(most);
            sl.seedItem.reserve(most);
        }
        const SearchArgs a = searchArgs(c, P, sl, b, r);
        SeedArgs sd = seedArgs(c, P, sl, b, r);
        // seeds on their own stream (sD), so that they run ahead of the FM
        // phase of the batch before (both are HBM-latency bound and light)
        if (r == 0) {
            SH_HIP(hipStreamWaitEvent(sD, sl.free, 0));
        } else {
            SH_HIP(hipStreamWaitEvent(sD, eventsOf(sl, r - 1).textDone, 0));
            launchRoundReset(sl.small.ptr, sl.queues.ptr, sD);
        }
        // streamed upload: the batch's patterns (packed here on the host while
        // the batches before it search; unpacked on sD ahead of its seeds)
        auto seeds = [&](uint32_t i0, uint32_t i1) {
            sd.itemBegin = i0;
            sd.nitems = i1;
            launchSeeds(sd, c->I.sigma, std::max<uint32_t>(1, std::min<uint32_t>((i1 - i0 + 1023) / 1024, (uint32_t)c->numCU * 8)), sD);
        };
        if (P.chunked0 && b == 0) {
            // (streamed, early text) the first chunk's seeds as soon as it is
            // up; the text phase starts on their tasks while the rest of the
            // batch uploads; the other chunks' seeds as each arrives (a lone
            // batch is four chunks: staging.cpp), then the FM phase
            const uint64_t step = c->up.rc ? 2 * c->up.chunk : c->up.chunk;
            const uint64_t p1 = std::min<uint64_t>(bstart[1], step);
            ensureUploaded(c, p1, sD);
            SH_HIP(hipEventRecord(sl.fmStart, sD));
            seeds(0, (uint32_t)(p1 * c->nsearch));
            seedTasksDone(sl);
            SH_HIP(hipEventRecord(sl.seedDone0, sD));
            // each later part's seed launch timed on its own (not the upload waits between)
            uint32_t part = 0;
            for (uint64_t p0 = p1; p0 < bstart[1]; p0 += step, ++part) {
                const uint64_t pe = std::min<uint64_t>(bstart[1], p0 + step);
                ensureUploaded(c, pe, sD);
                while (c->partEv.size() < 2 * (size_t)(part + 1)) c->partEv.emplace_back(hipEventDefault);
                SH_HIP(hipEventRecord(c->partEv[2 * part], sD));
                seeds((uint32_t)(p0 * c->nsearch), (uint32_t)(pe * c->nsearch));
                SH_HIP(hipEventRecord(c->partEv[2 * part + 1], sD));
            }
            sl.seedParts = part;
            sl.seedsInParts = true;
        } else {
            sl.seedsInParts = false;
            ensureUploaded(c, bstart[b + 1], sD);
            SH_HIP(hipEventRecord(ev.fmStart, sD));
            seeds(0, nitems);
            // the seed tasks end here: the text phase may start on them (a
            // lone device-resident batch's text phase waits for its FM phase:
            // published after it below)
            if (P.split && P.early) seedTasksDone(sl);
            SH_HIP(hipEventRecord(sl.seedDone0, sD));
        }
        SH_HIP(hipEventRecord(ev.seedDone, sD));
        SH_HIP(hipStreamWaitEvent(sA, ev.seedDone, 0));
        SH_HIP(hipEventRecord(ev.fmBegin, sA));
        launchSearch(a, c->I.sigma, c->edit, P.count, b == 0 && !P.early ? P.firstBlocks : P.blocks, P.fmLds, sA);
        SH_HIP(hipEventRecord(ev.fmDone, sA));
        ++S.search_launches;
    }

    // every round of batch b in turn
    void issueRounds(uint64_t b) {
        for (uint32_t r = 0; r < P.rounds; ++r) {
            issueFM(b, r);
            issueText(b, r);
        }
    }

    // one launch per batch (kSearchTextBatch) after its FM phase; the
    // first batch of an early pass in two: its seed tasks while its FM
    // phase runs, then the tasks the FM phase appended after them
    void issueText(uint64_t b, uint32_t r) {
        Ctx::Slot& sl = slotOf(b);
        const RoundEv ev = eventsOf(sl, r);
        const bool split0 = P.early && b == 0;  // (one round: ev is the slot's own events)
        sl.twoText = P.split && split0;
        SH_HIP(hipStreamWaitEvent(sB, split0 ? sl.seedDone0 : ev.fmDone, 0));
        SH_HIP(hipEventRecord(ev.textStart, sB));
        if (P.split) {
            TextBatchArgs t = textArgs(c, P, sl, b, r);
            if (split0) {
                t.taskCount = sl.small.ptr + kSwSeedTasks;
                launchTextBatch(t, c->edit, P.count, P.textBlocks, P.tx.lds, sB);
                SH_HIP(hipEventRecord(sl.textMid0, sB));
                SH_HIP(hipStreamWaitEvent(sB, sl.fmDone, 0));
                SH_HIP(hipEventRecord(sl.textMid1, sB));
                t.taskBegin = sl.small.ptr + kSwSeedTasks;
                t.taskCount = sl.small.ptr + kSwTaskCount;
                t.work = sl.queues.ptr + kQueueFmTasks;
                ++S.text_launches;
            }
            launchTextBatch(t, c->edit, P.count, P.textBlocks, P.tx.lds, sB);
            ++S.text_launches;
        }
        SH_HIP(hipEventRecord(ev.textDone, sB));
    }

    // the batch's kernel spans (Slot's events) into the stats, summed over its rounds
    void addSpans(Ctx::Slot& sl) {
        float ms = 0;
        for (uint32_t r = 0; r + 1 < P.rounds; ++r) {
            const RoundEv ev = eventsOf(sl, r);
            SH_HIP(hipEventElapsedTime(&ms, ev.fmStart, ev.seedDone));
            S.seed_ms += ms;
            SH_HIP(hipEventElapsedTime(&ms, ev.fmBegin, ev.fmDone));
            S.search_ms += ms;
            SH_HIP(hipEventElapsedTime(&ms, ev.textStart, ev.textDone));
            S.text_ms += ms;
        }
        if (sl.seedsInParts) {  // the seed launches, not the upload waits between them
            SH_HIP(hipEventElapsedTime(&ms, sl.fmStart, sl.seedDone0));
            for (uint32_t i = 0; i < sl.seedParts; ++i) {
                S.seed_ms += ms;
                SH_HIP(hipEventElapsedTime(&ms, c->partEv[2 * i], c->partEv[2 * i + 1]));
            }
        } else {
            SH_HIP(hipEventElapsedTime(&ms, sl.fmStart, sl.seedDone));
        }
        S.seed_ms += ms;
        SH_HIP(hipEventElapsedTime(&ms, sl.fmBegin, sl.fmDone));
        S.search_ms += ms;
        if (sl.twoText) {  // the two launches, not the wait for the FM phase between them
            SH_HIP(hipEventElapsedTime(&ms, sl.textStart, sl.textMid0));
            S.text_ms += ms;
            SH_HIP(hipEventElapsedTime(&ms, sl.textMid1, sl.textDone));
        } else {
            SH_HIP(hipEventElapsedTime(&ms, sl.textStart, sl.textDone));
        }
        S.text_ms += ms;
    }

    // A batch after its text phase, on stream sC: totals and overflow check,
    // locate and sort, the stages that are on, the sink. Returns false on
    // overflow; `finishCheck` then reads the locate flags and timings.
    bool finish(uint64_t b) {
        Ctx::Slot& sl = slotOf(b);
        const uint64_t q0 = P.bstart[b], nb = P.bstart[b + 1] - q0;
        BatchRecord& rec = c->pinned.ptr[b];
        c->mark("finish", b);
        if (!totals(sl, b, nb, rec)) return false;
        const bool direct = locateSort(sl, rec, q0, nb);  // (then, as with no rows, no stage runs: no whole hits)
        BatchView v{rec.rows && !direct ? c->out.ptr + c->nout : nullptr, rec.rows, c->qoff.ptr, (uint32_t)nb, q0,
                    c->stageScratch, c->tmp, &rec.kept, sC, false};
        stages(v, rec);
        // the rows that leave decide where they go (never direct after a stage: the sort stands)
        const BatchPlan d = decideBatch(batchIn(v.rows, nb));
        if (d.needRecs && v.rows) growOut(c->outRecs, c->nout + v.rows, c->nout);  // (the rescue may have added rows)
        SH_HIP(hipEventRecord(c->sortDone, sC));
        c->batchQ0.push_back(q0);
        c->batchEnd.push_back(c->nout + v.rows);
        c->batchDirect.push_back(d.direct ? 1 : 0);
        sinkBatch(q0, v.rows, d);
        launchLocateFlagsOut(c->small.ptr + kLocFlags, &rec.locateFlags, sC);
        SH_HIP(hipEventRecord(c->flagsDown, sC));
        if (P.sleepy) SH_HIP(hipEventRecord(c->flagsDownSleep, sC));
        c->nout += v.rows;
        S.hits += v.rows;
        return true;
    }

    // The batch's totals into its pinned record (the host waits for its text
    // phase) and the overflow check: false when a work buffer was too small.
    bool totals(Ctx::Slot& sl, uint64_t b, uint64_t nb, BatchRecord& rec) {
        // After the text phase, on sC (work on sB would wait for CU slots
        // between two text phases): the per-query row counts are scanned into
        // segment offsets right away, and one small kernel then writes the
        // batch's counters, its row total and its long-segment counts into
        // its record in pinned host memory: one host round trip per batch, not
        // two (until r5 the counters went up first, and the scan waited for
        // the host to check them). A batch whose buffers overflowed is redone
        // anyway, so its scan is wasted work, not wrong work.
        SH_HIP(hipStreamWaitEvent(sC, sl.textDone, 0));
        SH_HIP(hipEventRecord(c->locStart, sC));
        // (the chain's words of c->small are zero here: cleared at the pass's
        // start, and by kBatchTotals and kLocateFlagsOut once read)
        c->partial.reserve(scanTiles((uint32_t)nb));
        uint32_t* const segCounts = c->small.ptr + kLocSegCounts;
        querySegments(sl.qcnt.ptr, (uint32_t)nb, c->qoff.ptr, c->partial.ptr, c->big.ptr, segCounts, c->huge.ptr,
                      segCounts + 1, sC);
        launchBatchTotals(sl.small.ptr, sl.queues.ptr, c->qoff.ptr + nb, segCounts, rec.slot, sC);
        SH_HIP(hipEventRecord(P.sleepy ? c->totalsDownSleep : c->totalsDown, sC));
        if (P.sleepy) waitSleepy(c->totalsDownSleep, P.k.pollUs);
        else SH_HIP(hipEventSynchronize(c->totalsDown));
        c->mark("text done, rows", b);
        addSpans(sl);
        const uint32_t flags = rec.slot[kSwFlags];
        if (flags & kFlagStack) throw Error("search stack overflow (internal bound violated)");
        if (flags & kFlagTextStack) throw Error("text phase: internal stack bound violated");
        if (flags & (kFlagHits | kFlagTasks)) {  // hit or task buffer too small
            // (pipelined: issueFM may be reading the caps on the other host
            // thread; they grow after the pass, before the serial re-run)
            if (flags & kFlagTasks) growCap(P.serial ? c->taskCap : seenTask, rec.slot[kSwTaskCount]);
            if (flags & kFlagHits) growCap(P.serial ? c->hitCap : seenHit, rec.slot[kSwHitCount]);
            overflow = true;  // (the scan zeroed the slot's per-query counts, kBatchTotals its counters)
            freeSlot(sl, sC);
            return false;
        }
        S.cursors += rec.slot[kSwFilled];
        if (rec.rows >= (1ull << 32)) throw Error("more than 2^32 located hits in one batch of patterns");
        return true;
    }

    // What decideBatch (hit_route.h) is asked, twice per batch: before the
    // sort with the sorted rows (direct, needRecs: neither depends on the rows
    // when a stage is on), and after the last stage with the rows that leave.
    BatchIn batchIn(uint64_t rows, uint64_t nb) const {
        return {c->sk.route, c->sk.wholeFallback, c->sk.ok, c->nout, rows, nb, c->sk.cap, c->sk.limitN,
                c->more.empty(), Ctx::kDownSlot, c->loci.on, c->pairs.on};
    }

    // A device-resident output of the call (c->out, c->outRecs) grown to hold
    // `need` records, the first `keep` of what it holds kept
    template <typename Buf>
    void growOut(Buf& buf, uint64_t need, uint64_t keep) {
        if (need <= buf.cap) return;
        SH_HIP(hipStreamSynchronize(c->stF));  // sink copies may still read the old buffer
        buf.growKeeping(std::max<size_t>(need + need / 2, 1024), std::min<size_t>(keep, buf.cap), sC);
    }

    // locate: SA / LF locate into the segments that `totals` scanned, then the
    // canonical sort into the device-resident output: whole hits, or compact
    // records where the call's sink takes those (then it returns true).
    bool locateSort(Ctx::Slot& sl, const BatchRecord& rec, uint64_t q0, uint64_t nb) {
        // reserved slots incl. len-0 holes; a wave's last range may reach past
        // the capacity without having written there (no overflow flag)
        const uint64_t nh = std::min<uint64_t>(rec.slot[kSwHitCount], c->hitCap);
        const uint64_t rows = rec.rows;
        const uint32_t nbig = rec.nbig, nhuge = rec.nhuge;
        c->k0.reserve(std::max<uint64_t>(rows, 1));
        if (nhuge) c->k1.reserve(std::max<uint64_t>(rows, 1));
        launchLocate(locateArgs(c, sl, nh), P.count, sC);
        SH_HIP(hipEventRecord(c->locDone, sC));
        freeSlot(sl, sC);  // the slot's hits are consumed
        if (nhuge) c->tmp.reserve(bigSortTempBytes(rows, nhuge) + 256);
        // A batch whose sink takes compact records is sorted straight into
        // them: the record is the sort key with the batch-local query in
        // front, so nothing is decoded and nothing of the batch goes into
        // c->out (Ctx::wholeHits expands it should a reader of c->out ask).
        const BatchPlan d = decideBatch(batchIn(rows, nb));
        const uint64_t end = rows ? c->nout + rows : 0;  // (no rows: the sorts write nothing, nothing grows)
        if (d.needRecs) growOut(c->outRecs, end, c->nout);
        if (d.direct) {
            sortCompact(c->k0.ptr, c->k1.ptr, rows, c->qoff.ptr, (uint32_t)nb, c->big.ptr, nbig, c->huge.ptr, nhuge,
                        c->outRecs.ptr + c->nout, c->tmp.ptr, c->tmp.cap, sC);
            c->outStale = true;
        } else {
            growOut(c->out, end, c->nout);
            sortDecode(c->k0.ptr, c->k1.ptr, rows, c->qoff.ptr, (uint32_t)nb, c->big.ptr, nbig, c->huge.ptr, nhuge, q0,
                       c->I.dRecStarts.ptr, (uint32_t)c->I.recStarts.size(), c->out.ptr + c->nout, c->tmp.ptr,
                       c->tmp.cap, sC);
        }
        return d.direct;
    }

    // The stages that are on, in pass_plan.h's order, over the one view of the
    // batch's whole hits: the sink sees what the last one left. A stage that
    // is off, or finds no rows left at its turn, records no events and counts
    // no batch. v.later tells a stage that changes the records whether to
    // write their segments again (pass_plan.h, the segments rule). Each case
    // holds what is the stage's own: the rule's numbers, its buffers, its counts.
    void stages(BatchView& v, BatchRecord& rec) {
        const StagesOn on = stagesOn(c->loci.on, c->pairs.on, c->rescue.on, c->sk.limitN != 0);
        Ctx::StageStats& T = c->stageStats;
        for (uint32_t s = 0; s < kStages; ++s) {
            stageRan[s] = on.on[s] && v.rows != 0;
            if (!stageRan[s]) continue;
            v.later = laterStage(on, s);
            const Ctx::StageStats::Figures f = T.figures(s);
            if (f.batches) {
                ++*f.batches;
                SH_HIP(hipEventRecord(c->stageStart[s], sC));
            }
            switch (s) {
            case kStageLoci:  // docs/semantics.md "Loci": one record per locus
                T.loci.hits_in += v.rows;
                lociBatch(v, c->loci.window, c->loci.bufs);
                T.loci.loci += v.rows;
                break;
            case kStageRescue: {
                // docs/semantics.md "Mate rescue": the hits without a mate get their
                // fragment windows scanned for the partner's pattern, and what that
                // finds joins the batch's hits before the pair stage cuts them. The
                // batch may grow here, by no more than it has anchors: c->out grows
                // between the stage's halves, once the count is known, and keeps the
                // batch's records.
                const RescueIn in{c->m, c->pairs.minFrag, c->pairs.maxFrag, c->rescue.maxErr, c->rescue.maxAnchors,
                                  c->edit, c->I.dRecStarts.ptr, (uint32_t)c->I.recStarts.size(), c->I.n,
                                  c->I.text3.ptr, c->pats3.ptr + v.q0 * c->patBlocks, c->patBlocks};
                const uint64_t r = rescueFind(v, in, c->rescue.bufs, T.rescue);
                growOut(c->out, c->nout + v.rows + r, c->nout + v.rows);
                v.hits = c->out.ptr + c->nout;
                rescueMerge(v, r, c->rescue.bufs);
                break;
            }
            case kStagePairs: {
                // docs/semantics.md "Pairs": the hits with a mate in the batch, which holds whole pairs; in
                // best mode ("Best pairs") of those each pair's least-error placements, and `kept` counts
                // what leaves the stage either way
                const PairLinksOut links{&c->pairs.linkBuf, c->nout};
                const BestPairsIn best{c->pairs.delta, c->pairs.summary.ptr, c->pairs.linksOn ? &links : nullptr};
                T.pairs.hits_in += v.rows;
                pairsBatch(v, c->m, c->pairs.minFrag, c->pairs.maxFrag, c->pairs.bufs, &rec.pairs,
                           c->pairs.summaryOn ? &best : nullptr);
                T.pairs.kept += v.rows;
                break;
            }
            case kStageLimit:  // --max_hits: this batch's queries keep their n best positions (search_n)
                limitBatch(v, c->sk.limitN, c->limit);
                break;
            }
            if (f.batches) SH_HIP(hipEventRecord(c->stageDone[s], sC));
        }
    }

    // The call's host sink: the batch's hits (`rows` from c->nout on) go to
    // host memory on stF while later batches search, by the one copy that
    // decideBatch chose (hit_route.h); once a batch takes none, the rest of
    // the call's hits go after the pass. d.compactFirst: kCompactHits makes
    // the records from the whole hits in c->out; else the sort has written
    // them into c->outRecs (finish).
    void sinkBatch(uint64_t q0, uint64_t rows, const BatchPlan& d) {
        switch (d.copy) {
        case BatchCopy::None: break;
        case BatchCopy::RecordsDma:
            // compact records in HBM on sC (by the sort, or from the whole
            // hits: full grid, ~20 us), then one D2H copy on stF: a copy engine
            // moves them, no workgroup waits on PCIe writes beside the text phase
            if (d.compactFirst)
                launchCompactHits(c->out.ptr + c->nout, rows, q0, c->I.dRecStarts.ptr, c->outRecs.ptr + c->nout, sC,
                                  1u << 16);
            SH_HIP(hipEventRecord(c->recsMade, sC));
            SH_HIP(hipStreamWaitEvent(c->stF, c->recsMade, 0));
            SH_HIP(hipMemcpyAsync(c->sk.recs() + c->nout, c->outRecs.ptr + c->nout, rows * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, c->stF));
            break;
        case BatchCopy::ExpanderSlot: {  // 8-B records, expanded on the host (Expander)
            const uint64_t j = c->sk.downJobs++;
            const size_t slot = (size_t)(j % Ctx::kDownSlots);
            if (j >= Ctx::kDownSlots) c->expander->waitFor(j + 1 - Ctx::kDownSlots);  // the slot is read
            while (c->downEv.size() < Ctx::kDownSlots) c->downEv.emplace_back(hipEventDisableTiming);
            uint64_t* stage = c->downRing.ptr + slot * (Ctx::kDownSlot / sizeof(uint64_t));
            uint64_t* dev = c->outRecs.ptr + c->nout;
            if (d.compactFirst) {
                c->outC.reserve(Ctx::kDownSlots * (Ctx::kDownSlot / sizeof(uint64_t)));
                dev = c->outC.ptr + slot * (Ctx::kDownSlot / sizeof(uint64_t));
                launchCompactHits(c->out.ptr + c->nout, rows, q0, c->I.dRecStarts.ptr, dev, sC);
            }
            SH_HIP(hipEventRecord(c->recsMade, sC));
            SH_HIP(hipStreamWaitEvent(c->stF, c->recsMade, 0));
            SH_HIP(hipMemcpyAsync(stage, dev, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stF));
            SH_HIP(hipEventRecord(c->downEv[slot], c->stF));
            c->expander->submit({c->downEv[slot], stage, c->sk.hits() + c->nout, rows, q0});
            break;
        }
        case BatchCopy::WholeDma:
            SH_HIP(hipStreamWaitEvent(c->stF, c->sortDone, 0));
            SH_HIP(hipMemcpyAsync(c->sk.hits() + c->nout, c->out.ptr + c->nout, rows * sizeof(sahara_hit),
                                  hipMemcpyDeviceToHost, c->stF));
            break;
        }
        c->sk.ok = d.ok;
        if (d.ok) c->sk.done = c->nout + rows;
    }

    void finishCheck(uint64_t b) {
        if (P.sleepy) waitSleepy(c->flagsDownSleep, P.k.pollUs);  // recorded beside flagsDown
        SH_HIP(hipEventSynchronize(c->flagsDown));
        if (c->pinned.ptr[b].locateFlags & kFlagLocate) throw Error("locate walked off the SA samples (corrupt index)");
        float ms = 0;
        SH_HIP(hipEventElapsedTime(&ms, c->locStart, c->locDone));
        S.locate_ms += ms;
        SH_HIP(hipEventElapsedTime(&ms, c->locDone, c->sortDone));
        S.sort_ms += ms;
        for (uint32_t s = 0; s < kStages; ++s) {  // the stages that ran on the batch (finish(b + 1) records again after this)
            double* const total = c->stageStats.figures(s).kernelMs;
            if (!stageRan[s] || !total) continue;
            SH_HIP(hipEventElapsedTime(&ms, c->stageStart[s], c->stageDone[s]));
            *total += ms;
            // (flagsDown has passed the pair stage's last copy, the one into the batch's record)
            if (s == kStagePairs) c->stageStats.pairs.pairs += c->pinned.ptr[b].pairs;
            if (s == kStagePairs && c->pairs.linksOn && c->pairs.bufs.linkTimed) {
                SH_HIP(hipEventElapsedTime(&ms, c->pairs.bufs.linkStart, c->pairs.bufs.linkDone));
                c->stageStats.linkMs += ms;
            }
        }
        c->mark("checked", b);
    }
};

// count mode: the work counters into the stats; (P.probe) the first text
// launch's wave lives, (SAHARA_DUMP_COUNTERS) the raw counters to stderr
static void readCounters(Ctx* c, const PassPlan& P, sahara_stats& S, hipStream_t sC) {
    unsigned long long h[kCounters];
    auto per = [&](Counter sum, Counter n) { return (double)h[sum] / std::max(1.0, (double)h[n]); };
    if (P.probe) {
        SH_HIP(hipMemcpy(h, c->counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
        auto since = [&](Counter i) { return (h[i] - h[kCtBornMin]) / 100.0; };
        std::fprintf(stderr, "text wave lives (first launch, us): last start %.1f first end %.1f last end %.1f mean %.1f; "
                     "tasks all taken seen first %.1f last %.1f by %llu waves, which ran on %.1f on average\n",
                     since(kCtBornMax), since(kCtEndMin), since(kCtEndMax),
                     h[kCtLifeSum] / 100.0 / std::max<double>(1, S.text_grid * 4.0), since(kCtDryMin), since(kCtDryMax),
                     h[kCtDryWaves], per(kCtDryRun, kCtDryWaves) / 100.0);
        std::fprintf(stderr, "text iterations before / after: %llu (busy lanes %.1f) / %llu (busy lanes %.1f); "
                     "nodes stolen %llu\n",
                     h[kCtIterPre], per(kCtActPre, kCtIterPre), h[kCtIterPost], per(kCtActPost, kCtIterPost), h[kCtStolen]);
        std::fprintf(stderr, "text wall per iteration (us) before: refill %.2f steps+emit %.2f; after: refill %.2f steps+emit %.2f\n",
                     per(kCtWallPreRefill, kCtIterPre) / 100.0, per(kCtWallPreStep, kCtIterPre) / 100.0,
                     per(kCtWallPostRefill, kCtIterPost) / 100.0, per(kCtWallPostStep, kCtIterPost) / 100.0);
    }
    SH_HIP(hipMemcpyAsync(h, c->counters.ptr, sizeof(h), hipMemcpyDeviceToHost, sC));
    SH_HIP(hipStreamSynchronize(sC));
    static const std::pair<uint64_t sahara_stats::*, Counter> statOf[] = {
        {&sahara_stats::nodes, kCtNodes}, {&sahara_stats::rank_nodes, kCtRankNodes},
        {&sahara_stats::ext_lines, kCtExtLines}, {&sahara_stats::lf_steps, kCtLfSteps},
        {&sahara_stats::text_nodes, kCtTextNodes}, {&sahara_stats::conversions, kCtTextTasks},
        {&sahara_stats::fm_iterations, kCtFmIter}, {&sahara_stats::text_iterations, kCtTextIter},
        {&sahara_stats::text_active, kCtTextActive}, {&sahara_stats::text_refills, kCtTextRefills},
        {&sahara_stats::text_cycles_refill, kCtCyRefill}, {&sahara_stats::text_cycles_step, kCtCyStep},
        {&sahara_stats::text_cycles_emit, kCtCyEmit}, {&sahara_stats::text_compare_steps, kCtCompareSteps},
        {&sahara_stats::text_steps, kCtTextSteps}, {&sahara_stats::text_pos_tasks, kCtPosTasks},
        {&sahara_stats::text_stolen, kCtStolen}, {&sahara_stats::best_skipped, kCtBestSkipped}};
    for (const auto& so : statOf) S.*so.first = h[so.second];
    if (P.k.dump) {
        for (uint32_t i = 0; i < kCounters; ++i) std::fprintf(stderr, "%s%llu", i ? " " : "counters ", h[i]);
        std::fprintf(stderr, "\n");
    }
}

// One pass over the staged patterns in batches of <= 4M. Per batch:
//   stream stD: chunk unpack (streamed upload), kSeedItems
//   stream st : kSearchFM                    -> hits, tasks of its slot
//   stream stB: kSearchTextBatch             -> hits of its slot
//   stream stC: row counts + ranks, scan, locate, sort, decode
//   stream stF: the batch's hits to the host sink (streamed calls)
// Ctx::kSlots slots rotate, so the seeds and FM phase of later batches
// (memory-latency bound) overlap the text phase of batch i (ALU bound), the
// text phases run back to back, and locate and sort of batch i-1 fill the
// gaps on stream stC. The issuing thread runs seeds, FM(i), text(i) as soon as
// slot i % kSlots is free; the finisher thread runs finish(i) (locate, sort,
// download), which frees it. Buffer overflow is detected after the fact from
// each batch's flags; the whole pass is then redone on one stream with grown
// buffers (`redo`: serial), re-running a batch until it fits.
void runPass(Ctx* c, bool count, bool redo, sahara_stats& S, bool& overflow) {
    const PassPlan P = makePlan(c, count, redo);
    const uint64_t nbatch = P.nbatch();
    overflow = false;
    S.patterns = c->npat;
    S.search_grid = P.blocks;
    S.text_grid = P.split ? P.textBlocks : 0u;
    S.pipelined = P.serial ? 0u : 1u;
    S.best_rounds = P.rounds > 1 ? P.rounds : 0u;
    c->stack.reserve((size_t)P.stackLevels * std::max(P.blocks, P.firstBlocks) * 256);  // levels beyond the LDS part
    initWorkCaps(c, P.maxBatch, P.k);
    // Pinned, so that the records' copies are plain DMA writes: a copy into
    // pageable memory waited behind the streamed upload's copies (4.5 ms for
    // batch 0's row total at C3 over PCIe, r3)
    c->pinned.reserve(nbatch);
    reserveLocate(c, P.maxBatch, Ctx::kSlots);
    // The search kernels rank each hit's rows in its query's segment as they
    // write it (an atomic add on the slot's per-query count), so the locate
    // chain starts at the scan. Until r4 a pass of scattered atomics in the
    // chain (kCountRows) did it, beside the next batches' search, where the
    // chain lagged behind them: C3 805M -> 843M, C2 482M -> 503M, C5 94.2M ->
    // 95.6M reads/s (profiles/r04_emit_rank_ab.txt)
    for (auto& sl : c->slot) SH_HIP(hipMemsetAsync(sl.qcnt.ptr, 0, (P.maxBatch + 1) * sizeof(uint32_t), c->st));
    Pass ps{c, P, S, overflow, c->st, P.serial ? c->st : c->stB, P.serial ? c->st : c->stC, P.serial ? c->st : c->stD};
    auto syncAll = [&](std::initializer_list<hipStream_t> ss) {
        for (hipStream_t s : ss) SH_HIP(hipStreamSynchronize(s));
    };
    c->mark("pass", 0);
    syncAll({c->st, c->stB, c->stC, c->stD});
    c->mark("pass synced", 0);
    if (c->pairs.summaryOn)  // (a re-run after an overflow starts from the same: no copy of the first pass is in flight)
        std::fill_n(c->pairs.summary.ptr, c->pairs.summaryPairs, sahara_pair_summary{kBestNone, kBestNone, 0, 0, 0});
    if (count) {
        SH_HIP(hipMemsetAsync(c->counters.ptr, 0, kCounters * sizeof(unsigned long long), ps.sA));
        for (Counter minimum : {kCtBornMin, kCtEndMin, kCtDryMin})
            SH_HIP(hipMemsetAsync(c->counters.ptr + minimum, 0xFF, sizeof(unsigned long long), ps.sA));
    }
    c->nout = 0;
    c->sk.done = 0;
    c->sk.ok = sinkStarts(c->sk.route);
    c->batchQ0.clear();
    c->batchEnd.clear();
    c->batchDirect.clear();
    c->outStale = false;
    SH_HIP(hipMemsetAsync(c->small.ptr, 0, 8 * sizeof(uint32_t), ps.sC));  // the locate chain's words (finish)
    for (auto& sl : c->slot) ps.resetSlot(sl, ps.sA);
    for (auto& sl : c->slot)  // the earlier rounds' events (Pass::eventsOf), before the pass's threads start
        while (sl.earlier.size() + 1 < P.rounds) sl.earlier.emplace_back();

    if (!P.serial) {
        // Two host threads (host_pool.h issueAndFinish). This one packs the
        // queries of a streamed upload and issues seeds, FM(b) and text(b) as
        // soon as batch b's slot is free; a finisher thread waits for each
        // batch's text phase and issues its locate, sort and hit download, so
        // that batch b's hits leave while later batches are still being packed
        // and searched. FM(b) reuses the slot that finish(b - kSlots) released.
        bool pending = false;  // finishCheck owed for batch `owed`
        uint64_t owed = 0;
        auto setup = [&] {
            c->place.bind();
            if (P.k.timerSlackNs) prctl(PR_SET_TIMERSLACK, P.k.timerSlackNs, 0, 0, 0);
            SH_HIP(hipSetDevice(c->device));
        };
        auto issue = [&](uint64_t b) {
            c->mark("issue", b);
            ps.issueRounds(b);
            c->mark("issued", b);
            ++S.batches;
        };
        auto check = [&] { if (pending) ps.finishCheck(owed); };
        auto finish = [&](uint64_t f) {
            check();
            owed = f;
            return pending = ps.finish(f);  // false: the caller redoes the pass serially
        };
        issueAndFinish(nbatch, Ctx::kSlots, setup, issue, finish, check, [&] {
            c->mark("finisher joined", 0);
            syncAll({ps.sA, ps.sB, ps.sC, ps.sD, c->stF});
            c->mark("streams synced", 0);
        });
        if (overflow) {  // the caller redoes the pass serially with the grown buffers
            c->taskCap = std::max(c->taskCap, ps.seenTask);
            c->hitCap = std::max(c->hitCap, ps.seenHit);
            return;
        }
    } else {
        for (uint64_t b = 0; b < nbatch; ++b) {
            ++S.batches;
            for (;;) {  // re-run the batch until its buffers suffice
                overflow = false;
                ps.issueRounds(b);
                if (ps.finish(b)) {
                    ps.finishCheck(b);
                    break;
                }
            }
        }
        overflow = false;
        SH_HIP(hipStreamSynchronize(c->stF));
    }
    if (count) readCounters(c, P, S, ps.sC);
}

}  // namespace sahara
