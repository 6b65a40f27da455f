// Stand-alone check of pair_links_core.h (no HIP): the first record of a range
// that has the range's least err (bestRangeArgMin, from the per-block minima)
// against a linear scan that shares nothing with the header, over random errs
// in 0..3: every [lb, ub) of 0 to 300 records around block borders, and ranges
// with the minimum only in the left edge, only in one whole block, only in
// the right edge, and in several of those places at once; the primary key's
// order; pairMapq's whole table. tests/test_pair_links_core.py builds it under
// the address and undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../sahara_amd/csrc/pair_links_core.h"

using namespace sahara;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static uint64_t rngState = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
    rngState ^= rngState << 13;
    rngState ^= rngState >> 7;
    rngState ^= rngState << 17;
    return rngState;
}

struct Errs {
    std::vector<uint8_t> e, blk;
    mutable uint64_t reads = 0;
    void blocks() {
        blk.assign((e.size() + 63) / 64, 255);
        for (size_t i = 0; i < e.size(); ++i) blk[i / 64] = std::min(blk[i / 64], e[i]);
    }
    // the range's least err and its first index by a plain scan; then the header's, which must agree
    void check(uint64_t lb, uint64_t ub) const {
        uint32_t least = kBestNone;
        uint64_t first = ub;
        for (uint64_t j = lb; j < ub; ++j)
            if (e[j] < least) {
                least = e[j];
                first = j;
            }
        reads = 0;
        const auto errAt = [this](uint64_t j) {
            ++reads;
            return (uint32_t)e.at(j);  // (at: a read outside the records is caught)
        };
        const auto blockAt = [this](uint64_t b) {
            ++reads;
            return (uint32_t)blk.at(b);
        };
        CHECK(bestRangeMin(errAt, blockAt, lb, ub) == least);
        reads = 0;
        const uint64_t got = bestRangeArgMin(errAt, blockAt, lb, ub, least);
        if (got != first) std::fprintf(stderr, "[%llu, %llu): got %llu, want %llu\n", (unsigned long long)lb,
                                       (unsigned long long)ub, (unsigned long long)got, (unsigned long long)first);
        CHECK(got == first);
        CHECK(reads <= 126 + 64 + (ub > lb ? (ub - lb) / 64 : 0));
        // a value the range does not hold: none
        if (lb < ub && least > 0) CHECK(bestRangeArgMin(errAt, blockAt, lb, ub, least - 1) == ub);
    }
};

static Errs randomErrs(size_t n, uint32_t lo) {
    Errs E;
    E.e.resize(n);
    for (auto& x : E.e) x = (uint8_t)(lo + rnd() % (4 - lo));
    E.blocks();
    return E;
}

static void everyRange() {
    // 0 to 300 records from every start around the borders of the first blocks
    for (int round = 0; round < 3; ++round) {
        const Errs E = randomErrs(64 * 8 + 17, 0);
        for (uint64_t lb : {0ull, 1ull, 62ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 191ull, 192ull})
            for (uint64_t len = 0; len <= 300; ++len) E.check(lb, lb + len);
    }
    // mostly dear records, a few cheap ones: the minimum is rare, as in a tandem run
    for (int round = 0; round < 20; ++round) {
        Errs E = randomErrs(700, 2);
        for (int k = 0; k < 3; ++k) E.e[rnd() % E.e.size()] = (uint8_t)(rnd() % 2);
        E.blocks();
        for (int t = 0; t < 400; ++t) {
            const uint64_t lb = rnd() % E.e.size(), ub = lb + rnd() % (E.e.size() - lb + 1);
            E.check(lb, ub);
        }
    }
}

// [lb, ub) = [40, 300): left edge [40, 64), whole blocks 1..3 = [64, 256), right edge [256, 300)
static void planted() {
    const uint64_t lb = 40, ub = 300;
    struct Place {
        const char* what;
        std::vector<uint64_t> at;
        uint64_t want;
    };
    const Place places[] = {
        {"left edge only", {50}, 50},
        {"left edge, first record", {40}, 40},
        {"left edge, last record", {63}, 63},
        {"one whole block only: the first", {64}, 64},
        {"one whole block only: the middle", {150}, 150},
        {"one whole block only: the last record of the last", {255}, 255},
        {"right edge only", {270}, 270},
        {"right edge, first record", {256}, 256},
        {"right edge, last record", {299}, 299},
        {"left edge and right edge", {60, 290}, 60},
        {"whole block and right edge", {200, 256}, 200},
        {"left edge and whole block", {41, 64, 128}, 41},
        {"two whole blocks", {191, 130}, 130},
        {"twice in one block", {140, 135}, 135},
        {"everywhere", {45, 70, 140, 250, 280}, 45},
    };
    for (const Place& p : places) {
        Errs E = randomErrs(64 * 6, 1);  // errs 1..3; the planted minimum is 0
        // cheaper records outside the range, in the blocks the range shares: the edges' block minima mislead
        E.e[10] = 0;
        E.e[39] = 0;
        E.e[300] = 0;
        E.e[319] = 0;
        for (uint64_t j : p.at) E.e[j] = 0;
        E.blocks();
        const auto errAt = [&](uint64_t j) { return (uint32_t)E.e.at(j); };
        const auto blockAt = [&](uint64_t b) { return (uint32_t)E.blk.at(b); };
        const uint64_t got = bestRangeArgMin(errAt, blockAt, lb, ub, 0);
        if (got != p.want) std::fprintf(stderr, "%s: got %llu\n", p.what, (unsigned long long)got);
        CHECK(got == p.want);
        E.check(lb, ub);
    }
    // a range inside one block, and one across a border without a whole block
    Errs E = randomErrs(256, 1);
    E.e[70] = 0;
    E.e[100] = 0;
    E.e[130] = 0;
    E.blocks();
    E.check(71, 120);
    E.check(90, 135);
    E.check(101, 130);
    E.check(101, 131);
    E.check(64, 128);
    E.check(64, 64);
    E.check(200, 100);  // (lb > ub: empty)
}

static void keys() {
    CHECK(pairPrimaryKey(0, 7) < pairPrimaryKey(1, 0));
    CHECK(pairPrimaryKey(3, 7) < pairPrimaryKey(3, 8));
    CHECK(pairPrimaryKey(kBestNone - 1, 0xFFFFFFFFu) < kLinkNoKey);
    CHECK(pairPrimaryIndex(pairPrimaryKey(30, 0xFFFFFFFEu)) == 0xFFFFFFFEu);
    CHECK(pairPrimaryIndex(pairPrimaryKey(0, 0)) == 0);
}

static void mapq() {
    for (uint32_t best = 0; best <= 255; ++best)
        for (uint32_t next = 0; next <= 255; ++next) {
            if (best < kBestNone && next <= best) continue;  // next lies above best where both have a value
            for (uint32_t n = 0; n <= 70; ++n) {
                uint32_t want;
                if (best == 255 || n == 0) want = 0;
                else if (n >= 3) want = 0;
                else if (n == 2) want = 1;
                else if (next == 255) want = 60;
                else want = 10 * std::min<uint32_t>(next - best, 6);
                CHECK(pairMapq(best, next, n) == want);
            }
        }
    CHECK(pairMapq(0, 1, 1) == 10);
    CHECK(pairMapq(4, 255, 1) == 60);
    CHECK(pairMapq(0, 6, 1) == 60);
    CHECK(pairMapq(0, 5, 1) == 50);
    CHECK(pairMapq(2, 30, 1) == 60);
    CHECK(pairMapq(0, 1, 2) == 1);
    CHECK(pairMapq(0, 255, 3) == 0);
    CHECK(pairMapq(0, 255, 65535) == 0);
}

int main() {
    everyRange();
    planted();
    keys();
    mapq();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
