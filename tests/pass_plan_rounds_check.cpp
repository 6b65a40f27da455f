// The one geometry of a pass of several rounds (pass_plan.h worstRound)
// against values worked out by hand (test_best_plan.py): besthits plans its
// FM LDS and stack, its text geometry and its batch size for the most
// searches and the most errors of any round, and every round fits them.
#include <cstdio>
#include <vector>

#include "../sahara_amd/csrc/pass_plan.h"

using namespace sahara;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);   \
            ++failures;                                            \
        }                                                          \
    } while (0)

struct Round {
    uint32_t nsearch, maxErr;
};

int main() {
    CHECK(worstRound(std::vector<Round>{}).nsearch == 0 && worstRound(std::vector<Round>{}).maxErr == 0);
    const std::vector<Round> one{{3, 2}};
    CHECK(worstRound(one).nsearch == 3 && worstRound(one).maxErr == 2);  // one round: today's pass
    // pigeon j = 0..3 at length 60: 1, 2, 3, 4 searches; the most of both in the last round
    const std::vector<Round> pigeon{{1, 0}, {2, 1}, {3, 2}, {4, 3}};
    // ... and a list whose most searches and most errors sit in different rounds
    const std::vector<Round> mixed{{9, 0}, {2, 3}, {5, 1}};
    CHECK(worstRound(pigeon).nsearch == 4 && worstRound(pigeon).maxErr == 3);
    CHECK(worstRound(mixed).nsearch == 9 && worstRound(mixed).maxErr == 3);
    for (const auto& rounds : {pigeon, mixed}) {
        const WorstRound w = worstRound(rounds);
        const uint32_t m = 60, patBlocks = 2;
        const TextGeometry g = textGeometry(m, w.maxErr, patBlocks, w.nsearch);
        const size_t fmLds = fmLdsBytes(w.nsearch, m, 4);
        const uint64_t mb = maxBatchOf(std::nullopt, true, w.nsearch, false);
        for (const Round& r : rounds) {
            const TextGeometry gr = textGeometry(m, r.maxErr, patBlocks, r.nsearch);
            CHECK(gr.winBlocks <= g.winBlocks && gr.textStack <= g.textStack && gr.tableWords <= g.tableWords);
            CHECK(2 * r.nsearch * m <= g.tableWords);  // the round's table fits the LDS before the lane slots
            CHECK(gr.lds <= g.lds);
            CHECK(fmLdsBytes(r.nsearch, m, 4) <= fmLds);
            CHECK(fmStackCap(r.maxErr, 6) <= fmStackCap(w.maxErr, 6));
            CHECK(mb * r.nsearch <= 1ull << 31);  // a batch's work items of every round fit 2^31
        }
    }
    // m = 60: 3 errors need 66 symbols = 3 blocks, 0 errors 2; the plan takes 3
    CHECK(textGeometry(60, 3, 2, 4).winBlocks == 3 && textGeometry(60, 0, 2, 1).winBlocks == 2);
    CHECK(maxBatchOf(std::nullopt, false, worstRound(mixed).nsearch, false) == 1ull << 22);
    CHECK(maxBatchOf(std::nullopt, false, 4096, false) == 1ull << 19);
    if (!failures) std::puts("OK");
    return failures ? 1 : 0;
}
