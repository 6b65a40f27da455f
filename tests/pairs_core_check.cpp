// Stand-alone check of pairs_core.h and of hit_route.h's pairs field (no HIP):
// the range of a hit's mates, the record order, the mate test and the whole
// per-record decision (pairKeeps: one lower bound over the sorted records, the
// way kPairFlags of pairs.hip runs it) against a brute-force restatement of
// docs/semantics.md "Pairs" that compares every record with every other and
// shares nothing with the header: over records written by hand and over
// pseudo-random sorted records with positions below dmin, positions near 2^32,
// dmin == dmax == 0 and duplicate positions, searched over the whole batch and
// within the partner's segment. Then decideBatch with pairs = true on every
// route. tests/test_pairs_core.py builds it under the address and
// undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "../sahara_amd/csrc/hit_route.h"
#include "../sahara_amd/csrc/pairs_core.h"

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
    uint32_t seq_id, err;
    uint64_t pos;
};
using Rows = std::vector<Row>;
using Flags = std::vector<char>;

static void sortRows(Rows& h) {
    std::sort(h.begin(), h.end(), [](const Row& a, const Row& b) {
        return std::tie(a.qid, a.seq_id, a.pos, a.err) < std::tie(b.qid, b.seq_id, b.pos, b.err);
    });
}

struct At {
    const Rows* h;
    const Row& operator()(uint64_t i) const { return h->at(i); }  // (at: a search that leaves the records is caught)
};

// the header's decision per record; narrow: within the partner's segment, found as kLociSegments finds it
static Flags byCore(const Rows& h, uint32_t len, uint32_t minFrag, uint32_t maxFrag, bool narrow) {
    const PairDist d = pairDist(len, minFrag, maxFrag);
    Flags keep(h.size());
    for (size_t i = 0; i < h.size(); ++i) {
        uint64_t first = 0, last = h.size();
        if (narrow) {
            const uint64_t partner = pairPartner(h[i].qid);
            first = std::lower_bound(h.begin(), h.end(), partner, [](const Row& r, uint64_t q) { return r.qid < q; }) -
                    h.begin();
            last = std::lower_bound(h.begin(), h.end(), partner + 1, [](const Row& r, uint64_t q) { return r.qid < q; }) -
                   h.begin();
        }
        keep[i] = pairKeeps(At{&h}, h[i].qid, h[i].seq_id, h[i].pos, d.dmin, d.dmax, first, last);
    }
    return keep;
}

// the rule restated: a hit is kept iff some hit is concordant with it (fragments in 128 bits: no wrap anywhere)
static Flags restated(const Rows& h, uint32_t len, uint32_t minFrag, uint32_t maxFrag) {
    Flags keep(h.size(), 0);
    const unsigned __int128 least = minFrag > len ? minFrag : len;
    for (size_t i = 0; i < h.size(); ++i)
        for (size_t j = 0; j < h.size() && !keep[i]; ++j) {
            const Row &x = h[i], &y = h[j];
            if ((x.qid / 4 != y.qid / 4) || (x.qid % 4) + (y.qid % 4) != 3 || x.seq_id != y.seq_id) continue;
            const Row& fwd = x.qid % 2 == 0 ? x : y;
            const Row& rev = x.qid % 2 == 0 ? y : x;
            if (rev.pos < fwd.pos) continue;
            const unsigned __int128 frag = (unsigned __int128)rev.pos + len - fwd.pos;
            keep[i] = frag >= least && frag <= maxFrag;
        }
    return keep;
}

static void same(const Rows& h, uint32_t len, uint32_t minFrag, uint32_t maxFrag, int line) {
    const Flags want = restated(h, len, minFrag, maxFrag);
    for (bool narrow : {false, true})
        if (byCore(h, len, minFrag, maxFrag, narrow) != want) {
            std::fprintf(stderr, "%s:%d: len %u fragments [%u, %u] narrow %d: core and rule differ\n", __FILE__, line, len,
                         minFrag, maxFrag, (int)narrow);
            ++failures;
        }
}

static void checkPieces() {
    CHECK(pairPartner(0) == 3 && pairPartner(3) == 0 && pairPartner(1) == 2 && pairPartner(2) == 1);
    CHECK(pairPartner(4000000001ull) == 4000000002ull && pairPartner(44) == 47);
    CHECK(pairDist(48, 100, 300).dmin == 52 && pairDist(48, 100, 300).dmax == 252);
    CHECK(pairDist(48, 0, 48).dmin == 0 && pairDist(48, 0, 48).dmax == 0);  // min_fragment below len counts as len
    CHECK(pairDist(100, 0xFFFFFFFFu, 0xFFFFFFFFu).dmin == 0xFFFFFFFFull - 100);
    // the forward mate looks right, the reverse mate left, clipped at 0 before the subtraction
    PairRange r = pairRange(0, 1000, 52, 252);
    CHECK(r.any && r.lo == 1052 && r.hi == 1252);
    r = pairRange(3, 1000, 52, 252);
    CHECK(r.any && r.lo == 748 && r.hi == 948);
    r = pairRange(3, 100, 52, 252);
    CHECK(r.any && r.lo == 0 && r.hi == 48);
    r = pairRange(3, 52, 52, 252);
    CHECK(r.any && r.lo == 0 && r.hi == 0);
    CHECK(!pairRange(3, 51, 52, 252).any && !pairRange(1, 0, 1, 1).any && pairRange(1, 0, 0, 0).any);
    r = pairRange(2, 0xFFFFFFF0ull, 0xFFFFFF00ull, 0xFFFFFFFFull);  // near 2^32: the sums need 64 bits
    CHECK(r.any && r.lo == 0x1FFFFFEF0ull && r.hi == 0x1FFFFFFEFull);
    r = pairRange(0, ~0ull - 5, 3, 10);  // the end of the range saturates
    CHECK(r.any && r.lo == ~0ull - 2 && r.hi == ~0ull);
    CHECK(!pairRange(0, ~0ull - 5, 6, 10).any);
    CHECK(pairCompare(1, 2, 3, 1, 2, 3) == 0 && pairCompare(0, 9, 9, 1, 0, 0) < 0 && pairCompare(1, 1, 9, 1, 2, 0) < 0);
    CHECK(pairCompare(1, 2, 2, 1, 2, 3) < 0 && pairCompare(2, 0, 0, 1, 9, 9) > 0 && pairCompare(1, 3, 0, 1, 2, 9) > 0);
    CHECK(pairCompare(1, 2, 1ull << 40, 1, 2, 3) > 0);
    CHECK(pairIsMate(3, 1, 10, 3, 1, 10) && !pairIsMate(3, 1, 11, 3, 1, 10) && !pairIsMate(3, 2, 5, 3, 1, 10) &&
          !pairIsMate(4, 1, 5, 3, 1, 10));
}

static void checkHandWritten() {
    // A at 100, rc B at 152, 352 and 353, len 48: fragments 100, 300 and 301
    Rows edge = {{0, 0, 0, 100}, {3, 0, 0, 152}, {3, 0, 1, 352}, {3, 0, 2, 353}};
    CHECK((byCore(edge, 48, 100, 300, false) == Flags{1, 1, 1, 0}));
    CHECK((byCore(edge, 48, 101, 300, false) == Flags{1, 0, 1, 0}));
    CHECK((byCore(edge, 48, 101, 299, false) == Flags{0, 0, 0, 0}));
    CHECK((byCore(edge, 48, 301, 301, true) == Flags{1, 0, 0, 1}));
    // both mates at one position; duplicates are kept or dropped together
    Rows one = {{4, 1, 0, 7}, {4, 1, 1, 7}, {7, 1, 2, 7}, {7, 1, 2, 8}};
    CHECK((byCore(one, 48, 48, 48, false) == Flags{1, 1, 1, 0}));
    CHECK((byCore(one, 48, 0, 49, true) == Flags{1, 1, 1, 1}));
    CHECK((byCore(one, 48, 49, 49, false) == Flags{1, 1, 0, 1}));
    // rc mate left of the forward mate, another record, both forward, another pair's partner, the last record
    Rows none = {{0, 0, 0, 500}, {0, 1, 0, 100}, {2, 0, 0, 600}, {3, 0, 0, 300}, {7, 0, 0, 600}};
    CHECK((byCore(none, 48, 0, 1000, false) == Flags{0, 0, 0, 0, 0}));
    CHECK(byCore({}, 48, 0, 100, false).empty());
    for (const Rows* h : {&edge, &one, &none})
        for (uint32_t lo : {0u, 48u, 49u, 100u, 101u, 300u, 301u})
            for (uint32_t hi : {48u, 49u, 100u, 299u, 300u, 301u, 1000u})
                if (lo <= hi) same(*h, 48, lo, hi, __LINE__);
}

static void checkRandom() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return s % n;
    };
    // few pairs, two records, crowded positions (duplicates, positions below dmin), some near 2^32 and beyond
    Rows h;
    for (int i = 0; i < 1500; ++i) {
        const uint64_t where = rnd(4);
        const uint64_t pos = where == 0 ? rnd(40) : where == 1 ? 200 + rnd(400) : where == 2 ? 0xFFFFFF00ull + rnd(600)
                                                                                             : 3 * rnd(100);
        h.push_back({rnd(12), (uint32_t)rnd(2), (uint32_t)rnd(3), pos});
    }
    sortRows(h);
    size_t kept = 0;
    for (auto f : {std::pair<uint32_t, uint32_t>{0, 20}, {20, 20}, {0, 0}, {20, 60}, {100, 300}, {200, 200}, {0, 700},
                   {500, 0xFFFFFFFFu}, {0xFFFFFF00u, 0xFFFFFFFFu}, {0, 0xFFFFFFFFu}})
        for (uint32_t len : {0u, 20u, 48u}) {
            if (f.second < len) continue;
            same(h, len, f.first, f.second, __LINE__);
            for (char c : byCore(h, len, f.first, f.second, false)) kept += c;
        }
    CHECK(kept > 1000);  // (the settings above keep and drop)
    same(h, 20, 20, 20, __LINE__);  // dmin == dmax == 0
    // a long run of one position, and a partner segment that ends the records
    Rows run;
    for (int i = 0; i < 700; ++i) run.push_back({8, 0, (uint32_t)(i % 3), 1000});
    for (int i = 0; i < 700; ++i) run.push_back({11, 0, 0, 1000 + (uint64_t)(i / 7)});
    sortRows(run);
    same(run, 48, 48, 48, __LINE__);
    same(run, 48, 100, 120, __LINE__);
    same(run, 48, 148, 148, __LINE__);
}

static void checkRoutes() {
    constexpr uint64_t kSlot = 64u << 20;
    for (HitRoute route : {HitRoute::Device, HitRoute::PinnedWhole, HitRoute::Expander, HitRoute::Records})
        for (bool fallback : {false, true})
            for (bool ok : {false, true})
                for (uint64_t nout : {0ull, 1000ull})
                    for (uint64_t cap : {0ull, 1500ull, 1ull << 30})
                        for (uint64_t nb : {4ull, 1ull << 28})
                            for (bool onePart : {false, true})
                                for (uint32_t limitN : {0u, 3u})
                                    for (bool loci : {false, true}) {
                                        const uint64_t rowsOf[] = {0, 1, 400, 600, kSlot / 8, kSlot / 8 + 1};
                                        BatchPlan first{};
                                        for (size_t r = 0; r < 6; ++r) {
                                            BatchIn in{route, fallback, ok,      nout,  rowsOf[r], nb,
                                                       cap,   limitN,   onePart, kSlot, loci,      true};
                                            const BatchPlan d = decideBatch(in);
                                            CHECK(!d.direct);
                                            CHECK(d.needRecs == (route == HitRoute::Records));
                                            if (r == 0) first = d;
                                            CHECK(d.needRecs == first.needRecs && d.direct == first.direct);  // whatever the rows
                                            // the copies are those the loci stage chooses for the same batch
                                            BatchIn l{route, fallback, ok, nout, rowsOf[r], nb, cap, limitN, onePart, kSlot, true};
                                            const BatchPlan e = decideBatch(l);
                                            CHECK(d.copy == e.copy && d.compactFirst == e.compactFirst && d.ok == e.ok &&
                                                  d.needRecs == e.needRecs && d.direct == e.direct);
                                        }
                                    }
    // the field defaults to off: the aggregate initialisers of before mean what they meant
    const BatchIn plain{HitRoute::Records, false, true, 0, 100, 12, 1000, 0, true, kSlot};
    CHECK(!plain.pairs && !plain.loci && decideBatch(plain).direct);
    BatchIn on = plain;
    on.pairs = true;
    CHECK(!decideBatch(on).direct && decideBatch(on).compactFirst && decideBatch(on).copy == BatchCopy::RecordsDma);
}

int main() {
    checkPieces();
    checkHandWritten();
    checkRandom();
    checkRoutes();
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
