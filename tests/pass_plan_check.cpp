// The HIP-free part of a pass's plan (pass_plan.h) against values worked out
// by hand from the rules it states (test_host_pool.py): batch boundaries, the
// ramp lists, the text window and stack sizes, the batch size, the stage order
// and the segments rule, the knobs.
#include <cstdio>
#include <cstdlib>

#include "../sahara_amd/csrc/pass_plan.h"

using namespace sahara;
using V = std::vector<uint64_t>;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);   \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    // batch boundaries (maxBatch 4)
    CHECK(batchStarts(10, 4, {}, {}, false) == (V{0, 3, 6, 10}));
    CHECK(batchStarts(0, 4, {}, {}, false) == (V{0}));
    CHECK(batchStarts(20, 4, {2, 3}, {1}, false) == (V{0, 2, 5, 8, 12, 15, 19, 20}));
    CHECK(batchStarts(9, 4, {2, 3}, {1}, false) == (V{0, 3, 6, 9}));  // too few patterns: ramps dropped
    CHECK(batchStarts(10, 4, {2, 3}, {1}, false) == (V{0, 2, 5, 9, 10}));  // just enough: 6 + one middle batch
    for (const V& head : {V{}, V{2, 3}, V{9}, V{1, 1, 1, 1}})
        for (const V& tail : {V{}, V{1}, V{4, 9}})
            for (uint64_t npat : {0, 1, 4, 5, 20, 21})  // serial: ramps dropped, whatever they are
                CHECK(batchStarts(npat, 4, head, tail, true) == batchStarts(npat, 4, {}, {}, false));
    for (uint64_t npat : {13, 14, 40}) {  // an oversized ramp entry is cut to maxBatch
        CHECK(batchStarts(npat, 4, {9}, {}, false) == batchStarts(npat, 4, {4}, {}, false));
        CHECK(batchStarts(npat, 4, {9}, {}, false)[1] == 4);
        CHECK(batchStarts(npat, 4, {}, {9}, false) == batchStarts(npat, 4, {}, {4}, false));
    }
    // ramp lists
    CHECK(parseRamp("2,3") == (V{2, 3}));
    CHECK(parseRamp("2:3") == (V{2, 3}));
    CHECK(parseRamp("0,5") == (V{5}));
    CHECK(parseRamp("x") == V{});
    CHECK(parseRamp("") == V{} && parseRamp(nullptr) == V{});
    // text window and stack: m = 100, k = 2; m + 2k = 224 and 225
    const TextGeometry a = textGeometry(100, 2, 4, 3);
    CHECK(a.exactWindow && a.winBlocks == 4 && a.textStack == 6);
    CHECK(a.tableWords == kTextTableMin);  // 2 * 3 * 100 words < one block of lane words
    CHECK(a.lds == 768 * 4 + 256 * (3 * (4 + 4) + 2 * 6) * 4);
    CHECK(textGeometry(100, 2, 4, 8).tableWords == 1600);
    const TextGeometry b = textGeometry(220, 2, 7, 3), b8 = textGeometry(220, 2, 8, 3), b9 = textGeometry(220, 2, 9, 3);
    CHECK(b.exactWindow && b.winBlocks == 7 && b8.exactWindow && b8.winBlocks == 7);
    CHECK(!b9.exactWindow && b9.winBlocks == (224 + 62) / 32);  // patBlocks > 8: block-aligned start
    const TextGeometry d = textGeometry(221, 2, 7, 3);
    CHECK(!d.exactWindow && d.winBlocks == 8 && d.winBlocks == (225 + 62) / 32);
    // the read lengths at which the geometry changes (tests/test_text_variants.py
    // runs the kernels at each): {m, k, patBlocks = ceil(m / 32)} ->
    // exactWindow, winBlocks; textStack = 2k + 2 throughout
    struct Edge { uint32_t m, k, pat; bool exact; uint32_t win; };
    for (const Edge& e : {
             Edge{96, 2, 3, true, 4},     // 100 symbols in 4 blocks, pattern 3 blocks
             Edge{97, 2, 4, true, 4},     // pattern 4 blocks: the shape of m = 100
             Edge{124, 2, 4, true, 4},    // m + 2k = 128: the 4 blocks filled to the last symbol
             Edge{125, 2, 4, true, 5},    // 129: a fifth block
             Edge{128, 0, 4, true, 4},    // window = pattern = 4 full blocks
             Edge{126, 1, 4, true, 4},
             Edge{220, 2, 7, true, 7},    // 224: 7 blocks copied from 8 loads
             Edge{221, 2, 7, false, 8},   // 225: 8 exact blocks would need 9 loads
             Edge{225, 0, 8, false, 8},   // (225 + 62) / 32
             Edge{225, 1, 8, false, 9},   // 227: (227 + 62) / 32, the 9 / 8 shape's lower end (226)
             Edge{250, 3, 8, false, 9},
             Edge{251, 3, 8, false, 9},   // 257: its upper end
             Edge{252, 3, 8, false, 10},  // 258: (258 + 62) / 32
             Edge{256, 0, 8, false, 9},   // pattern 8 full blocks
             Edge{257, 0, 9, false, 9},   // pattern 9 blocks
             Edge{640, 2, 20, false, 22}, Edge{672, 2, 21, false, 23}, Edge{673, 2, 22, false, 23}}) {
        CHECK((e.m + 31) / 32 == e.pat);
        const TextGeometry g = textGeometry(e.m, e.k, e.pat, 3);
        if (g.exactWindow != e.exact || g.winBlocks != e.win || g.textStack != 2 * e.k + 2) {
            std::fprintf(stderr, "m %u k %u: exact %d blocks %u stack %u\n", e.m, e.k, (int)g.exactWindow, g.winBlocks,
                         g.textStack);
            ++failures;
        }
    }
    CHECK(textGeometry(226 - 2, 1, 7, 3).winBlocks == 9 && textGeometry(226 - 2, 1, 7, 3).exactWindow == false);
    // the largest text phase that fits the 160 KB of LDS: three searches, k = 2.
    // table 2 * 3 * m words; lanes 256 * (3 * (window + pattern blocks) + 2 * 6) words
    CHECK(textGeometry(640, 2, 20, 3).lds == 3840 * 4 + 256 * (3 * (22 + 20) + 12) * 4);
    CHECK(textGeometry(640, 2, 20, 3).lds == 156672);
    CHECK(textGeometry(672, 2, 21, 3).lds == 4032 * 4 + 256 * (3 * (23 + 21) + 12) * 4);
    CHECK(textGeometry(672, 2, 21, 3).lds == 163584 && 163584 <= 160 * 1024 && 160 * 1024 - 163584 == 256);
    CHECK(textGeometry(673, 2, 22, 3).lds == 4038 * 4 + 256 * (3 * (23 + 22) + 12) * 4);
    CHECK(textGeometry(673, 2, 22, 3).lds == 166680 && 166680 > 160 * 1024);
    CHECK(textGeometry(128, 0, 4, 3).tableWords == kTextTableMin && textGeometry(129, 0, 5, 3).tableWords == 774);
    // FM phase
    CHECK(fmLdsBytes(5, 80, 0) == 400 * 4 && fmLdsBytes(5, 80, 8) == 400 * 4 + 8 * 4096);  // m = 80, five searches
    CHECK(fmLdsBytes(5, 80, 1) == 400 * 4 + 4096);
    CHECK(fmLdsBytes(7, 80, 0) == 560 * 4 && fmLdsBytes(7, 80, 8) == 560 * 4 + 8 * 4096);  // h2-k3, 0..3 errors: seven
    for (uint32_t sigma : {4u, 5u, 6u}) {
        CHECK(fmStackCap(0, sigma) == fmStackCap(1, sigma) && fmStackCap(1, sigma) == 2 * sigma);
        CHECK(fmStackCap(3, sigma) == 3 * (2 * sigma - 2) + 2);
    }
    CHECK(fmLdsBytes(3, 50, 0) == 152 * 4 && fmLdsBytes(3, 50, 4) == 152 * 4 + 4 * 4096);  // 150 words, rounded to 4
    // batch size
    CHECK(maxBatchOf(std::nullopt, true, 1, false) == 1ull << 21);
    CHECK(maxBatchOf(std::nullopt, false, 1, false) == 1ull << 22);
    CHECK(maxBatchOf(std::nullopt, false, 1024, false) == 1ull << 21);  // 2^31 / nsearch
    CHECK(maxBatchOf(std::nullopt, true, 3000, false) == (1ull << 31) / 3000);
    CHECK(maxBatchOf(0, true, 1, false) == 1);
    CHECK(maxBatchOf(333, false, 4, true) == 333);
    CHECK(maxBatchOf(1L << 40, false, 4, false) == 1ull << 29);
    CHECK(maxBatchOf(1L << 40, false, 1, true) == 1ull << 27);  // compact records
    CHECK(maxBatchOf(std::nullopt, false, 1, true) == 1ull << 22);
    CHECK(firstWorkCap(1) == 1u << 20 && firstWorkCap(1ull << 21) == 1u << 24 && firstWorkCap(1ull << 40) == 1u << 30);
    // The stages of a batch's sorted hits: their order, which of them are on,
    // and "a later stage runs" (the one rule for rewriting the per-query
    // segments) against the three expressions that decided it per stage
    // before, written out as they stood, with the pair stage's searches within
    // the segments (`narrow`: the path that is left). All 12 valid settings.
    CHECK(kStageLoci == 0 && kStageRescue == 1 && kStagePairs == 2 && kStageLimit == 3 && kStages == 4);
    int settings = 0;
    for (bool lociOn : {false, true})
        for (int mates : {0, 1, 2})  // pairs off, pairs on, pairs + rescue
            for (uint32_t limitN : {0u, 3u}) {
                const bool pairsOn = mates >= 1, rescueOn = mates == 2, narrow = true;
                const StagesOn on = stagesOn(lociOn, pairsOn, rescueOn, limitN != 0);
                CHECK(on.on[kStageLoci] == lociOn && on.on[kStageRescue] == rescueOn);
                CHECK(on.on[kStagePairs] == pairsOn && on.on[kStageLimit] == (limitN != 0));
                // the loci call site: `segments ? qoff : nullptr`
                const bool lociSegments = limitN || (pairsOn && narrow) || rescueOn;
                CHECK(laterStage(on, kStageLoci) == lociSegments);
                // the pairs call site: `limitN || narrow ? qoff : nullptr`, `rewrite = limitN != 0`
                const bool pairsQoff = limitN || narrow, pairsRewrite = limitN != 0;
                CHECK(laterStage(on, kStagePairs) == (pairsQoff && pairsRewrite));
                // the rescue wrote them again whenever it added records: the pair stage follows it
                if (rescueOn) CHECK(laterStage(on, kStageRescue));
                CHECK(!laterStage(on, kStageLimit));
                ++settings;
            }
    CHECK(settings == 12);
    for (bool lociOn : {false, true})  // the rescue with pairs off counts as off
        for (bool limit : {false, true}) {
            const StagesOn on = stagesOn(lociOn, false, true, limit);
            CHECK(!on.on[kStageRescue] && !on.on[kStagePairs]);
            CHECK(laterStage(on, kStageLoci) == limit && laterStage(on, kStageRescue) == limit);
        }
    // knobs: read on every call, defaults restored when unset
    for (const char* name : {"SAHARA_SPLIT", "SAHARA_PIPELINE", "SAHARA_BATCH", "SAHARA_RAMP", "SAHARA_FM_STEAL_AT",
                             "SAHARA_FM_LDS_DEPTH", "SAHARA_HITCAP", "SAHARA_REFILL_AT", "SAHARA_TEXT_STEPS",
                             "SAHARA_STEAL_AT", "SAHARA_POLL_US", "SAHARA_TIMER_SLACK_NS", "SAHARA_CHUNK_SEEDS",
                             "SAHARA_KMER_POS", "SAHARA_SEED_TASKS", "SAHARA_DUMP_COUNTERS", "SAHARA_TASKCAP",
                             "SAHARA_FM_BPC", "SAHARA_TEXT_BPC", "SAHARA_RAMP_END"})
        unsetenv(name);
    PassKnobs k = readPassKnobs(true);
    CHECK(k.split == 1 && k.pipeline && !k.batch && k.rampHead.empty() && k.fmStealAt == 0 && k.fmLdsDepth == 0);
    CHECK(k.textSteps == 2 && k.refillAt == 8 && k.stealAt == 8 && k.pollUs == 20 && k.timerSlackNs == 1000);
    CHECK(k.chunkSeeds && k.kmerPos && k.seedTasks && !k.dump && k.hitCap == 0 && k.taskCap == 0 && !k.fmBpc && !k.textBpc);
    k = readPassKnobs(false);  // the reference execution's defaults
    CHECK(k.fmStealAt == 8 && k.fmLdsDepth == 4);
    setenv("SAHARA_SPLIT", "0", 1);
    setenv("SAHARA_PIPELINE", "0", 1);
    setenv("SAHARA_BATCH", "333", 1);
    setenv("SAHARA_RAMP", "2:3", 1);
    setenv("SAHARA_FM_STEAL_AT", "99", 1);
    setenv("SAHARA_FM_LDS_DEPTH", "-1", 1);
    setenv("SAHARA_HITCAP", "0", 1);
    setenv("SAHARA_REFILL_AT", "100", 1);
    k = readPassKnobs(true);
    CHECK(k.split == 0 && !k.pipeline && k.batch && *k.batch == 333 && k.rampHead == (V{2, 3}));
    CHECK(k.fmStealAt == 64 && k.fmLdsDepth == 0 && k.hitCap == 1 && k.refillAt == 64);
    unsetenv("SAHARA_SPLIT");
    unsetenv("SAHARA_PIPELINE");
    k = readPassKnobs(true);
    CHECK(k.split == 1 && k.pipeline);
    if (!failures) std::puts("OK");
    return failures ? 1 : 0;
}
