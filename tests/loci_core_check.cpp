// Stand-alone check of loci_core.h and of hit_route.h's loci field (no HIP):
// the head predicate and the (err, index) key run sequentially, the way the
// kernels of loci.hip use them (flags, running locus number, minimum key per
// locus, gather), over rows written by hand and over 10^4 pseudo-random
// sorted rows, against a plain restatement of docs/semantics.md "Loci" that
// keeps a current representative and shares nothing with the header. Then
// decideBatch with loci = true on every route. tests/test_loci_core.py builds
// it under the address and undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "../sahara_amd/csrc/hit_route.h"
#include "../sahara_amd/csrc/loci_core.h"

using namespace sahara;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Row {
    uint64_t qid;
    uint32_t seq, err;
    uint64_t pos;
    bool operator==(const Row& o) const { return qid == o.qid && seq == o.seq && err == o.err && pos == o.pos; }
};
using Rows = std::vector<Row>;

// the stage's steps, one after the other, with the header's functions
static Rows byCore(const Rows& h, uint32_t W) {
    const size_t n = h.size();
    std::vector<uint32_t> num(n);
    uint32_t loci = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool head = i == 0 || lociHead(h[i - 1].qid, h[i - 1].seq, h[i - 1].pos, h[i].qid, h[i].seq, h[i].pos, W);
        loci += head ? 1u : 0u;
        num[i] = loci;
    }
    std::vector<uint64_t> best(loci, kLociNoKey);
    for (size_t i = 0; i < n; ++i) best[num[i] - 1] = std::min(best[num[i] - 1], lociKey(h[i].err, (uint32_t)i));
    Rows out;
    for (uint32_t l = 0; l < loci; ++l) out.push_back(h[lociKeyIndex(best[l])]);
    return out;
}

// the rule restated: walk the rows, keep the locus's best row so far
static Rows restated(const Rows& h, uint32_t W) {
    Rows out;
    for (size_t i = 0; i < h.size(); ++i) {
        bool fresh = i == 0;
        if (!fresh) {
            const Row& p = h[i - 1];
            if (p.qid != h[i].qid) fresh = true;
            else if (p.seq != h[i].seq) fresh = true;
            else if (h[i].pos > p.pos && h[i].pos - p.pos > (uint64_t)W) fresh = true;
        }
        if (fresh) out.push_back(h[i]);
        else if (h[i].err < out.back().err) out.back() = h[i];
    }
    return out;
}

static void checkHandWritten() {
    // gap exactly W against W + 1
    const Rows gap = {{0, 0, 2, 10}, {0, 0, 1, 13}, {0, 0, 0, 17}};
    CHECK((byCore(gap, 3) == Rows{{0, 0, 1, 13}, {0, 0, 0, 17}}));
    CHECK((byCore(gap, 4) == Rows{{0, 0, 0, 17}}));
    CHECK(byCore(gap, 2) == gap);
    // equal pos with different e
    const Rows dup = {{0, 0, 1, 5}, {0, 0, 2, 5}, {0, 0, 2, 5}, {0, 0, 0, 9}, {0, 0, 1, 9}};
    CHECK((byCore(dup, 0) == Rows{{0, 0, 1, 5}, {0, 0, 0, 9}}));
    CHECK((byCore(dup, 3) == Rows{{0, 0, 1, 5}, {0, 0, 0, 9}}));
    CHECK((byCore(dup, 4) == Rows{{0, 0, 0, 9}}));
    // a tie in e at two positions: the smaller pos
    const Rows tie = {{3, 1, 2, 100}, {3, 1, 1, 101}, {3, 1, 2, 101}, {3, 1, 1, 102}, {3, 1, 2, 103}};
    CHECK((byCore(tie, 1) == Rows{{3, 1, 1, 101}}));
    // a change of seq_id with a small gap, a change of qid, positions that fall
    const Rows change = {{0, 0, 1, 50}, {0, 1, 0, 51}, {1, 1, 0, 51}, {1, 1, 1, 52}, {2, 0, 2, 0}};
    CHECK((byCore(change, 10) == Rows{{0, 0, 1, 50}, {0, 1, 0, 51}, {1, 1, 0, 51}, {2, 0, 2, 0}}));
    const Rows falls = {{0, 0, 0, 900}, {0, 1, 0, 2}, {1, 0, 0, 1}};
    CHECK(byCore(falls, 5) == falls);
    // W = 0, empty input, the widest window
    const Rows w0 = {{0, 0, 2, 1}, {0, 0, 2, 1}, {0, 0, 1, 2}, {0, 0, 0, 3}};
    CHECK((byCore(w0, 0) == Rows{{0, 0, 2, 1}, {0, 0, 1, 2}, {0, 0, 0, 3}}));
    CHECK(byCore({}, 3).empty());
    CHECK((byCore(gap, 0xFFFFFFFFu) == Rows{{0, 0, 0, 17}}));
    // positions beyond 2^32 (a multi-part record) and the key's halves
    const Rows far = {{5, 0, 1, (1ull << 33)}, {5, 0, 0, (1ull << 33) + 2}, {5, 0, 0, (1ull << 34)}};
    CHECK((byCore(far, 2) == Rows{{5, 0, 0, (1ull << 33) + 2}, {5, 0, 0, (1ull << 34)}}));
    CHECK(lociKey(0, 0xFFFFFFFFu) < lociKey(1, 0) && lociKey(3, 7) < lociKey(3, 8));
    CHECK(lociKeyIndex(lociKey(15, 0xFFFFFFFEu)) == 0xFFFFFFFEu && lociKey(0xFFFFFFFFu, 0xFFFFFFFEu) < kLociNoKey);
    for (const Rows* r : {&gap, &dup, &tie, &change, &falls, &w0, &far})
        for (uint32_t W : {0u, 1u, 2u, 3u, 4u, 10u}) CHECK(byCore(*r, W) == restated(*r, W));
}

static void checkRandom() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return s % n;
    };
    Rows h;
    for (int i = 0; i < 10000; ++i)  // few queries, two records, crowded positions, duplicates
        h.push_back({rnd(40), (uint32_t)rnd(2), (uint32_t)rnd(4), rnd(2) ? rnd(300) : 1000 + 7 * rnd(40)});
    std::sort(h.begin(), h.end(), [](const Row& a, const Row& b) {
        return std::tie(a.qid, a.seq, a.pos, a.err) < std::tie(b.qid, b.seq, b.pos, b.err);
    });
    size_t last = h.size() + 1;
    for (uint32_t W : {0u, 1u, 2u, 3u, 5u, 6u, 7u, 50u, 1000u}) {
        const Rows a = byCore(h, W), b = restated(h, W);
        CHECK(a == b);
        CHECK(!a.empty() && a.size() <= last);  // a wider window never makes more loci
        last = a.size();
    }
    CHECK(byCore(h, 1000).size() == 80 && byCore(h, 0).size() > 2000);
}

static void checkRoutes() {
    constexpr uint64_t kSlot = 64u << 20;
    for (HitRoute route : {HitRoute::Device, HitRoute::PinnedWhole, HitRoute::Expander, HitRoute::Records})
        for (bool fallback : {false, true})
            for (bool ok : {false, true})
                for (uint64_t nout : {0ull, 1000ull})
                    for (uint64_t cap : {0ull, 1500ull, 1ull << 30})
                        for (uint64_t nb : {1ull, 1ull << 28})
                            for (bool onePart : {false, true})
                                for (uint32_t limitN : {0u, 3u}) {
                                    const uint64_t rowsOf[] = {0, 1, 400, 600, kSlot / 8, kSlot / 8 + 1};
                                    BatchPlan first{};
                                    for (size_t r = 0; r < 6; ++r) {
                                        BatchIn in{route, fallback, ok, nout, rowsOf[r], nb, cap, limitN, onePart, kSlot};
                                        in.loci = true;
                                        const BatchPlan d = decideBatch(in);
                                        CHECK(!d.direct);
                                        CHECK(d.needRecs == (route == HitRoute::Records));
                                        if (r == 0) first = d;
                                        CHECK(d.needRecs == first.needRecs && d.direct == first.direct);  // whatever the rows
                                        // the copies are those --max_hits 1 chooses for the same batch
                                        BatchIn lim{route, fallback, ok, nout, rowsOf[r], nb, cap, 1u, onePart, kSlot};
                                        const BatchPlan e = decideBatch(lim);
                                        CHECK(d.copy == e.copy && d.compactFirst == e.compactFirst && d.ok == e.ok &&
                                              d.needRecs == e.needRecs && d.direct == e.direct);
                                    }
                                }
    // the field defaults to off: the aggregate initialisers of before mean what they meant
    const BatchIn plain{HitRoute::Records, false, true, 0, 100, 10, 1000, 0, true, kSlot};
    CHECK(!plain.loci && decideBatch(plain).direct);
    BatchIn on = plain;
    on.loci = true;
    CHECK(!decideBatch(on).direct && decideBatch(on).compactFirst && decideBatch(on).copy == BatchCopy::RecordsDma);
}

int main() {
    checkHandWritten();
    checkRandom();
    checkRoutes();
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
