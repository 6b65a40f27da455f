// compact_hit_check.cpp — the host decoder of compact hit records
// (sahara_amd/csrc/compact_hit.h) against a plain lookup per record: an
// upper_bound over the record starts and over the block ends for every hit,
// no cursor. Built alone under the sanitizers (tests/test_compact_hit.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../sahara_amd/csrc/compact_hit.h"

using namespace sahara_compact;

namespace {

int g_failed = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

struct Hit {
    uint64_t qid, seq, pos;
    uint32_t err;
    bool operator==(const Hit& o) const { return qid == o.qid && seq == o.seq && pos == o.pos && err == o.err; }
};

uint64_t pack(uint64_t relQid, uint64_t text, uint32_t err) { return relQid << 36 | text << 4 | err; }

struct Blocks {
    std::vector<uint64_t> recs, end, qid0;
};

// the reference: every hit looked up from scratch
Hit plain(const Blocks& B, const std::vector<uint64_t>& S, uint64_t k) {
    const uint64_t v = B.recs[k], g = (v >> 4) & 0xFFFFFFFFull;
    const uint64_t blk = (uint64_t)(std::upper_bound(B.end.begin(), B.end.end(), k) - B.end.begin());
    const uint64_t seq = (uint64_t)(std::upper_bound(S.begin(), S.end() - 1, g) - S.begin()) - 1;  // (S ends with the text length)
    return {B.qid0[blk] + (v >> 36), seq, g - S[seq], (uint32_t)(v & 15u)};
}

// the decoder over [lo, hi), as the writers and the expander use it
std::vector<Hit> decode(const Blocks& B, const std::vector<uint64_t>& S, uint64_t nStarts, uint64_t lo, uint64_t hi) {
    std::vector<Hit> out;
    if (lo >= hi) return out;
    BlockCursor blk(B.end.data(), B.qid0.data(), B.end.size(), lo);
    RecordCursor rec(S.data(), nStarts);
    for (uint64_t k = lo; k < hi; ++k) {
        const uint64_t v = B.recs[k], pos = rec.seek(textOf(v));
        out.push_back({blk.qid0Of(k) + qidOf(v), rec.seq, pos, errOf(v)});
    }
    return out;
}

// every range [lo, hi) of the hits, with the text length as the last start and without it
void checkAllRanges(const Blocks& B, const std::vector<uint64_t>& S) {
    const uint64_t n = B.recs.size();
    for (uint64_t lo = 0; lo <= n; ++lo)
        for (uint64_t hi = lo; hi <= n; ++hi)
            for (uint64_t nStarts : {S.size(), S.size() - 1}) {
                const std::vector<Hit> got = decode(B, S, nStarts, lo, hi);
                CHECK(got.size() == hi - lo);
                for (uint64_t k = lo; k < hi && k - lo < got.size(); ++k) CHECK(got[k - lo] == plain(B, S, k));
            }
}

}  // namespace

int main() {
    CHECK(qidOf(pack(5, 0xFFFFFFFFull, 15)) == 5 && textOf(pack(5, 0xFFFFFFFFull, 15)) == 0xFFFFFFFFull &&
          errOf(pack(5, 0xFFFFFFFFull, 15)) == 15);
    CHECK(qidOf(pack((1ull << 28) - 1, 0, 0)) == (1ull << 28) - 1 && textOf(pack((1ull << 28) - 1, 0, 0)) == 0);

    // three records of 9, 1 and 20 symbols, a delimiter after each: starts 0, 10, 12, and the text length 33
    const std::vector<uint64_t> S = {0, 10, 12, 33};
    Blocks B;
    // block 0 (qids from 100): a record's first and last position, the last record's first and last, and
    // back to a lower record at a qid change
    B.recs = {pack(0, 0, 1),  pack(0, 8, 0),  pack(0, 10, 2), pack(0, 12, 0), pack(0, 31, 3),
              pack(1, 3, 0),  pack(1, 12, 1), pack(2, 0, 0),
              // block 1 (qids from 200) starts mid-record and goes down within its first qid change
              pack(0, 20, 0), pack(0, 21, 4), pack(3, 10, 0), pack(3, 30, 15),
              // block 3 (block 2 is empty; qids from 400)
              pack(0, 5, 0),  pack(7, 6, 0)};
    B.end = {8, 12, 12, 14};
    B.qid0 = {100, 200, 300, 400};
    checkAllRanges(B, S);
    {  // by hand, so that the reference is not the only witness
        const std::vector<Hit> all = decode(B, S, S.size(), 0, B.recs.size());
        CHECK((all[1] == Hit{100, 0, 8, 0}) && (all[2] == Hit{100, 1, 0, 2}) && (all[4] == Hit{100, 2, 19, 3}));
        CHECK((all[5] == Hit{101, 0, 3, 0}) && (all[8] == Hit{200, 2, 8, 0}) && (all[11] == Hit{203, 2, 18, 15}));
        CHECK((all[12] == Hit{400, 0, 5, 0}) && (all[13] == Hit{407, 0, 6, 0}));
        CHECK((decode(B, S, S.size(), 9, 10)[0] == Hit{200, 2, 9, 4}));  // a first lookup mid-record, mid-block
    }

    // an empty first block, two empty blocks in the middle, an empty last block
    Blocks E = B;
    E.end = {0, 8, 8, 8, 12, 14, 14};
    E.qid0 = {50, 100, 150, 160, 200, 400, 900};
    checkAllRanges(E, S);
    CHECK((decode(E, S, S.size(), 0, 1)[0] == Hit{100, 0, 0, 1}) && (decode(E, S, S.size(), 8, 9)[0] == Hit{200, 2, 8, 0}));

    // a single record, a single block
    const std::vector<uint64_t> S1 = {0, 41};
    Blocks O;
    O.recs = {pack(0, 0, 0), pack(0, 39, 1), pack(1, 0, 0), pack(1, 17, 2)};
    O.end = {4};
    O.qid0 = {0};
    checkAllRanges(O, S1);
    CHECK((decode(O, S1, 1, 1, 2)[0] == Hit{0, 0, 39, 1}));

    if (g_failed) std::fprintf(stderr, "%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
