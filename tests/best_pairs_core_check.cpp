// Stand-alone check of best_pairs_core.h (no HIP): the index range of a
// record's mates (bestMateRange: two bounds over the sorted records, the way
// kBestScore of pairs.hip runs it), the least err of a range from the per-block
// minima (bestRangeMin) and the keep test, against brute force that shares
// nothing with the header: pseudo-random sorted records, 1 to 400 of them,
// with duplicate positions, positions near 0 and near 2^64, and windows from
// one position to everything; ranges that are empty, of 1, 63, 64, 65 and 129
// records and of more than 3 whole blocks, that start and end exactly on block
// boundaries, with the minimum only in the head, only in the tail or only in
// one middle block. It also counts the reads of a range query against the
// bound 126 + range / 64. tests/test_best_pairs_core.py builds it under the
// address and undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "../sahara_amd/csrc/best_pairs_core.h"

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

struct At {
    const Rows* h;
    const Row& operator()(uint64_t i) const { return h->at(i); }  // (at: a search that leaves the records is caught)
};

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rngState ^= rngState << 13;
    rngState ^= rngState >> 7;
    rngState ^= rngState << 17;
    return rngState;
}

// ---- the range query: errs with their block minima, counted reads
struct Errs {
    std::vector<uint8_t> e, blk;
    mutable uint64_t reads = 0;
    explicit Errs(std::vector<uint8_t> v) : e(std::move(v)), blk((e.size() + 63) / 64, 255) {
        for (size_t i = 0; i < e.size(); ++i) blk[i / 64] = std::min(blk[i / 64], e[i]);
    }
    uint32_t query(uint64_t lb, uint64_t ub) const {
        reads = 0;
        return bestRangeMin([&](uint64_t j) { ++reads; return (uint32_t)e.at(j); },
                            [&](uint64_t b) { ++reads; return (uint32_t)blk.at(b); }, lb, ub);
    }
    uint32_t brute(uint64_t lb, uint64_t ub) const {
        uint32_t m = kBestNone;
        for (uint64_t j = lb; j < ub; ++j) m = std::min<uint32_t>(m, e[j]);
        return m;
    }
    void check(uint64_t lb, uint64_t ub) const {
        CHECK(query(lb, ub) == brute(lb, ub));
        CHECK(reads <= 126 + (ub > lb ? (ub - lb) / 64 : 0));
    }
};

static void rangeMinByHand() {
    // 400 records of err 5, one cheaper record planted where the case wants it
    auto with = [](std::vector<size_t> cheap) {
        std::vector<uint8_t> v(400, 5);
        for (size_t at : cheap) v[at] = 2;
        return Errs(v);
    };
    const Errs flat = with({});
    for (uint64_t lb : {0ull, 1ull, 63ull, 64ull, 65ull, 130ull})
        for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull, 200ull, 257ull})  // 200 from 64: blocks 1, 2, 3 whole
            if (lb + n <= 400) flat.check(lb, lb + n);
    CHECK(flat.query(7, 7) == kBestNone && flat.query(9, 3) == kBestNone);
    // [70, 330): head 70..127, whole blocks 2, 3, 4 (128..319), tail 320..329
    CHECK(with({71}).query(70, 330) == 2);    // only in the head
    CHECK(with({325}).query(70, 330) == 2);   // only in the tail
    CHECK(with({200}).query(70, 330) == 2);   // only in a middle block
    CHECK(with({69}).query(70, 330) == 5 && with({330}).query(70, 330) == 5);  // just outside
    CHECK(with({64 + 63}).query(64, 320) == 2 && with({319}).query(64, 320) == 2);  // exactly on block boundaries
    CHECK(with({63}).query(64, 320) == 5 && with({320}).query(64, 320) == 5);
    CHECK(with({100}).query(64, 128) == 2 && with({100}).query(65, 128) == 2 && with({100}).query(64, 127) == 2);
    // a block minimum outside the range's part of a partial block must not leak in
    CHECK(with({64}).query(65, 200) == 5 && with({199}).query(65, 199) == 5);
    // the early end at 0: a 0 in the head ends the query without a block read
    std::vector<uint8_t> z(400, 3);
    z[66] = 0;
    const Errs zero(z);
    CHECK(zero.query(65, 400) == 0 && zero.reads == 2);
}

static void rangeMinRandom() {
    for (int round = 0; round < 300; ++round) {
        const size_t n = 1 + rnd() % 400;
        std::vector<uint8_t> v(n);
        const uint32_t floor = rnd() % 3 ? 1 : 0;  // (with no 0 about, nothing ends early)
        for (auto& x : v) x = (uint8_t)(floor + rnd() % 6);
        if (rnd() % 2) v[rnd() % n] = 0;
        const Errs E(v);
        for (int k = 0; k < 60; ++k) {
            uint64_t a = rnd() % (n + 1), b = rnd() % (n + 1);
            if (rnd() % 4 == 0) a = a / 64 * 64;
            if (rnd() % 4 == 0) b = b / 64 * 64;
            E.check(std::min(a, b), std::max(a, b));
        }
        E.check(0, n);
    }
}

// ---- the mate range: against every record compared with every other
static void sortRows(Rows& h) {
    std::sort(h.begin(), h.end(), [](const Row& a, const Row& b) {
        return std::tie(a.qid, a.seq_id, a.pos, a.err) < std::tie(b.qid, b.seq_id, b.pos, b.err);
    });
}

static bool concordant(const Row& x, const Row& y, uint64_t dmin, uint64_t dmax) {
    if ((x.qid ^ 3ull) != y.qid || x.seq_id != y.seq_id) return false;
    const Row& f = (x.qid & 1) ? y : x;  // the even qid is the forward mate
    const Row& r = (x.qid & 1) ? x : y;
    if (r.pos < f.pos) return false;
    const unsigned __int128 d = (unsigned __int128)r.pos - f.pos;
    return d >= dmin && d <= dmax;
}

static void mateRanges(const Rows& h, uint64_t dmin, uint64_t dmax, bool narrow) {
    for (size_t i = 0; i < h.size(); ++i) {
        uint64_t first = 0, last = h.size();
        if (narrow) {
            const uint64_t partner = h[i].qid ^ 3ull;
            first = std::lower_bound(h.begin(), h.end(), partner, [](const Row& r, uint64_t q) { return r.qid < q; }) -
                    h.begin();
            last = std::upper_bound(h.begin(), h.end(), partner, [](uint64_t q, const Row& r) { return q < r.qid; }) -
                   h.begin();
        }
        const BestRange r = bestMateRange(At{&h}, h[i].qid, h[i].seq_id, h[i].pos, dmin, dmax, first, last);
        CHECK(r.lb <= r.ub && r.ub <= h.size());
        uint32_t least = kBestNone;
        for (size_t j = 0; j < h.size(); ++j) {
            const bool mate = concordant(h[i], h[j], dmin, dmax);
            CHECK(mate == (j >= r.lb && j < r.ub));
            if (mate) least = std::min(least, h[j].err);
        }
        CHECK((r.lb == r.ub) == !pairKeeps(At{&h}, h[i].qid, h[i].seq_id, h[i].pos, dmin, dmax, first, last));
        // the score over the range, by the block minima of the whole array
        std::vector<uint8_t> e(h.size());
        for (size_t j = 0; j < h.size(); ++j) e[j] = (uint8_t)h[j].err;
        const Errs E(e);
        CHECK(bestScore(h[i].err, E.query(r.lb, r.ub)) == (least == kBestNone ? kBestNone : h[i].err + least));
    }
}

static void mateRangesRandom() {
    for (int round = 0; round < 120; ++round) {
        const size_t n = 1 + rnd() % 400;
        const uint64_t base = round % 5 == 4 ? ~0ull - 300 : round % 5 == 3 ? 0 : 1000;  // near 2^64, near 0, inside
        const uint64_t span = 1 + rnd() % 300;
        const uint32_t pairs = 1 + rnd() % 3;
        Rows h(n);
        for (auto& r : h) r = {4 * (rnd() % pairs) + rnd() % 4, (uint32_t)(rnd() % 2), (uint32_t)(rnd() % 4), base + rnd() % span};
        sortRows(h);
        const uint64_t dmin = rnd() % 4 == 0 ? 0 : rnd() % 50;
        const uint64_t dmax = round % 7 == 0 ? dmin : round % 7 == 1 ? ~0ull - 1 : dmin + rnd() % 400;
        mateRanges(h, dmin, dmax, false);
        mateRanges(h, dmin, dmax, true);
    }
    // one query's 400 records at 40 positions against its partner's: ranges of many blocks
    Rows h;
    for (uint32_t i = 0; i < 200; ++i) h.push_back({0, 0, i % 3, 100 + i / 5});
    for (uint32_t i = 0; i < 200; ++i) h.push_back({3, 0, 1 + i % 2, 120 + i / 5});
    h[250].err = 0;
    sortRows(h);
    mateRanges(h, 0, 1000, true);
    mateRanges(h, 20, 25, true);
}

static void keepTest() {
    CHECK(bestKeeps(true, 3, 3, 0) && !bestKeeps(true, 4, 3, 0) && bestKeeps(true, 4, 3, 1));
    CHECK(!bestKeeps(false, 3, 3, 0) && !bestKeeps(false, 3, 3, 30));
    CHECK(!bestKeeps(true, kBestNone, 0, 30) && !bestKeeps(true, kBestNone, kBestNone, 0));
    CHECK(bestKeeps(true, 30, 0, kBestMaxDelta) && bestKeeps(true, 0, 0, 0));
    CHECK(bestScore(2, kBestNone) == kBestNone && bestScore(15, 15) == 30 && bestScore(0, 0) == 0);
}

int main() {
    rangeMinByHand();
    rangeMinRandom();
    mateRangesRandom();
    keepTest();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
