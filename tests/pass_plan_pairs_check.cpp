// Stand-alone check of pass_plan.h's batch granularity (no HIP): with
// granularity 4 (the pair stage: a pair's four qids stay in one batch) every
// boundary of batchStarts is a multiple of 4, the boundaries cover [0, npat),
// no batch is empty and none exceeds maxBatchOf's value, which is SAHARA_BATCH
// rounded down to a multiple of 4 and 4 where that leaves nothing; with
// granularity 1, given or defaulted, both functions return what they returned
// before they had the parameter (restated below, word for word). And
// cli/shard.h's granularity: shards of whole pairs.
// tests/test_pass_plan_pairs.py builds it under the sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <optional>
#include <vector>

#include "../sahara_amd/cli/shard.h"
#include "../sahara_amd/csrc/pass_plan.h"

using namespace sahara;
using V = std::vector<uint64_t>;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// the two functions as they were without a granularity
static uint64_t maxBatchBefore(std::optional<long> batch, bool streaming, uint32_t nsearch, bool compactRecs) {
    const uint64_t most = (1ull << 31) / nsearch;
    uint64_t mb = std::min<uint64_t>(streaming ? 1ull << 21 : 1ull << 22, most);
    if (batch) mb = std::max<uint64_t>(1, std::min<uint64_t>(most, (uint64_t)*batch));
    return compactRecs ? std::min<uint64_t>(mb, 1ull << 27) : mb;
}
static V startsBefore(uint64_t npat, uint64_t maxBatch, V head, V tail, bool serial) {
    V bstart{0};
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

static const V kNpat = {4, 8, 12, 1028};
static const V kBatch = {1, 3, 7, 257, 1ull << 21};
static const std::vector<V> kRamps = {{}, {1}, {2, 3}, {5}, {6, 9, 30}, {4, 8}, {257}, {1ull << 30}};

static void checkGranularity4() {
    for (uint64_t batch : kBatch)
        for (bool streaming : {false, true})
            for (bool compact : {false, true}) {
                const uint64_t mb = maxBatchOf((long)batch, streaming, 4, compact, 4);
                CHECK(mb % 4 == 0 && mb >= 4);
                CHECK(mb == (batch < 4 ? 4 : batch / 4 * 4));
                for (uint64_t npat : kNpat)
                    for (const V& head : kRamps)
                        for (const V& tail : kRamps)
                            for (bool serial : {false, true}) {
                                const V b = batchStarts(npat, mb, head, tail, serial, 4);
                                CHECK(b.size() >= 2 && b.front() == 0 && b.back() == npat);
                                for (size_t i = 0; i < b.size(); ++i) CHECK(b[i] % 4 == 0);
                                for (size_t i = 1; i < b.size(); ++i) CHECK(b[i] > b[i - 1] && b[i] - b[i - 1] <= mb);
                            }
            }
    CHECK(maxBatchOf(std::nullopt, true, 1, false, 4) == 1ull << 21);
    CHECK(maxBatchOf(std::nullopt, false, 3000, false, 4) == (1ull << 31) / 3000 / 4 * 4);
    // by hand: SAHARA_BATCH=7 is 4 with pairs on; ramps of 2 and 9 patterns are one and two pairs
    CHECK(maxBatchOf(7, true, 1, false, 4) == 4);
    CHECK(batchStarts(12, 4, {}, {}, false, 4) == (V{0, 4, 8, 12}));
    CHECK(batchStarts(1028, 256, {}, {}, false, 4) == (V{0, 204, 408, 616, 820, 1028}));
    CHECK(batchStarts(40, 8, {2, 9}, {6}, false, 4) == (V{0, 4, 12, 20, 28, 36, 40}));
    CHECK(batchStarts(12, 8, {2, 9}, {6}, false, 4) == (V{0, 4, 12}));  // too few patterns: the ramps are dropped
    CHECK(batchStarts(0, 4, {}, {}, false, 4) == (V{0}));
}

static void checkGranularity1() {
    for (uint64_t batch : kBatch)
        for (bool streaming : {false, true})
            for (bool compact : {false, true})
                for (uint32_t nsearch : {1u, 4u, 3000u}) {
                    const uint64_t was = maxBatchBefore((long)batch, streaming, nsearch, compact);
                    CHECK(maxBatchOf((long)batch, streaming, nsearch, compact) == was);
                    CHECK(maxBatchOf((long)batch, streaming, nsearch, compact, 1) == was);
                    CHECK(maxBatchOf(std::nullopt, streaming, nsearch, compact, 1) ==
                          maxBatchBefore(std::nullopt, streaming, nsearch, compact));
                    for (uint64_t npat : {0ull, 1ull, 4ull, 8ull, 9ull, 10ull, 12ull, 20ull, 1028ull, 1031ull})
                        for (const V& head : kRamps)
                            for (const V& tail : kRamps)
                                for (bool serial : {false, true}) {
                                    const V want = startsBefore(npat, was, head, tail, serial);
                                    CHECK(batchStarts(npat, was, head, tail, serial) == want);
                                    CHECK(batchStarts(npat, was, head, tail, serial, 1) == want);
                                }
                }
}

static void checkShards() {
    using sahara_cli::queryShard;
    for (size_t nreads : {2u, 6u, 10u, 238u})
        for (unsigned devices : {1u, 2u, 3u, 8u}) {
            size_t next = 0;
            for (unsigned g = 0; g < devices; ++g) {
                const auto s = queryShard(2 * nreads, 2, devices, g, 2);
                CHECK(s.r0 == next && s.r0 % 2 == 0 && s.r1 % 2 == 0 && s.q0 == 2 * s.r0 && s.q1 == 2 * s.r1);
                next = s.r1;
                const auto plain = queryShard(2 * nreads, 2, devices, g), same = queryShard(2 * nreads, 2, devices, g, 1);
                CHECK(plain.r0 == nreads * g / devices && plain.r1 == nreads * (g + 1) / devices);
                CHECK(same.r0 == plain.r0 && same.r1 == plain.r1 && same.q0 == plain.q0 && same.q1 == plain.q1);
            }
            CHECK(next == nreads);
        }
    // --limit_queries 8 of 10 reads in pairs: two pairs, split 1 + 1
    const auto a = queryShard(8, 2, 2, 0, 2), b = queryShard(8, 2, 2, 1, 2);
    CHECK(a.r0 == 0 && a.r1 == 2 && a.q1 == 4 && b.r0 == 2 && b.r1 == 4 && b.q0 == 4 && b.q1 == 8);
}

int main() {
    checkGranularity4();
    checkGranularity1();
    checkShards();
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
