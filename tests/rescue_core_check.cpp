// Stand-alone check of rescue_core.h and of align_core.h's split table build
// (no HIP): the window of a record at position 0, at the record's end and
// with a saturating dmax; the anchor test beside its neighbour; the order of
// the (errors, start) words; and alignTable / alignTrace / alignOne against a
// plain dynamic program of docs/semantics.md "Alignments" on pseudo-random
// small inputs, for every bound, with and without edit operations, the way
// kRescueScan of rescue.hip calls the table build: with a falling bound.
// tests/test_rescue_core.py builds it under the address and
// undefined-behaviour sanitizers and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../sahara_amd/csrc/align_core.h"
#include "../sahara_amd/csrc/rescue_core.h"

using namespace sahara;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void windows() {
    // an even qid looks to the right: [pos + dmin, pos + dmax], clipped to the record's last symbol
    RescueWindow w = rescueWindow(0, 10, 52, 304, 1000);
    CHECK(w.any && w.lo == 62 && w.hi == 314);
    w = rescueWindow(4, 900, 52, 304, 1000);
    CHECK(w.any && w.lo == 952 && w.hi == 999);
    w = rescueWindow(4, 947, 52, 304, 1000);
    CHECK(w.any && w.lo == 999 && w.hi == 999);
    CHECK(!rescueWindow(4, 948, 52, 304, 1000).any);  // begins at the '$'
    CHECK(!rescueWindow(4, 0, 0, 10, 0).any);          // an empty record
    w = rescueWindow(0, 0, 0, 0, 1);
    CHECK(w.any && w.lo == 0 && w.hi == 0);
    // dmax saturates: the sum would wrap
    w = rescueWindow(2, 5, 1, ~0ull, 100);
    CHECK(w.any && w.lo == 6 && w.hi == 99);
    w = rescueWindow(2, ~0ull - 3, 2, ~0ull, ~0ull);
    CHECK(w.any && w.lo == ~0ull - 1 && w.hi == ~0ull - 1);
    CHECK(!rescueWindow(2, ~0ull - 3, 4, ~0ull, ~0ull).any);
    // an odd qid looks to the left: [pos - dmax, pos - dmin], clipped at 0
    w = rescueWindow(3, 400, 52, 304, 1000);
    CHECK(w.any && w.lo == 96 && w.hi == 348);
    w = rescueWindow(3, 120, 52, 304, 1000);
    CHECK(w.any && w.lo == 0 && w.hi == 68);
    w = rescueWindow(1, 52, 52, 304, 1000);
    CHECK(w.any && w.lo == 0 && w.hi == 0);
    CHECK(!rescueWindow(1, 51, 52, 304, 1000).any);
    w = rescueWindow(1, 5, 0, ~0ull, 3);  // (a hit past the record's symbols is the caller's error: the window still clips)
    CHECK(w.any && w.lo == 0 && w.hi == 2);
}

static void anchorTest() {
    // (isFirst, prev, record, hasMate, dmin, dmax, recLen)
    CHECK(rescueIsAnchor(true, 0, 0, 0, 8, 1, 100, false, 52, 304, 1000));
    CHECK(!rescueIsAnchor(true, 0, 0, 0, 8, 1, 100, true, 52, 304, 1000));          // it has a mate
    CHECK(!rescueIsAnchor(false, 8, 1, 100, 8, 1, 100, false, 52, 304, 1000));      // a duplicate of its position
    CHECK(rescueIsAnchor(true, 8, 1, 100, 8, 1, 100, false, 52, 304, 1000));        // (i == 0: the neighbour is not read)
    CHECK(rescueIsAnchor(false, 8, 1, 99, 8, 1, 100, false, 52, 304, 1000));
    CHECK(rescueIsAnchor(false, 8, 0, 100, 8, 1, 100, false, 52, 304, 1000));
    CHECK(rescueIsAnchor(false, 7, 1, 100, 8, 1, 100, false, 52, 304, 1000));
    CHECK(!rescueIsAnchor(false, 7, 1, 100, 8, 1, 960, false, 52, 304, 1000));      // no window
    CHECK(!rescueIsAnchor(false, 7, 1, 100, 9, 1, 40, false, 52, 304, 1000));
}

static void order() {
    CHECK(rescueKey(0, 0) < rescueKey(0, 1) && rescueKey(0, 4095) < rescueKey(1, 0));
    CHECK(rescueKey(8, 4095) < kRescueNone);
    CHECK(rescueBest(rescueKey(3, 10), rescueKey(3, 9)) == rescueKey(3, 9));   // ties: the smaller start
    CHECK(rescueBest(rescueKey(2, 200), rescueKey(3, 9)) == rescueKey(2, 200));  // the fewer errors first
    CHECK(rescueBest(kRescueNone, rescueKey(8, 7)) == rescueKey(8, 7));
    CHECK(rescueKeyErr(rescueKey(8, 4095)) == 8 && rescueKeyAt(rescueKey(8, 4095)) == 4095);
    CHECK(kRescueMaxWindow - 1 <= 0xFFFFu);
}

// ---- the table build against a plain DP

struct Blocks {  // symbols as 3-bit-plane blocks; blocks past the end are zero (the text's pad, the pattern's mask)
    std::vector<Planes3> b;
    explicit Blocks(const std::vector<uint8_t>& s) : b(s.size() / 32 + 3, Planes3{0, 0, 0}) {
        for (size_t i = 0; i < s.size(); ++i) {
            Planes3& p = b[i / 32];
            const uint32_t bit = 1u << (i % 32);
            if (s[i] & 1) p.b0 |= bit;
            if (s[i] & 2) p.b1 |= bit;
            if (s[i] & 4) p.b2 |= bit;
        }
    }
    Planes3 operator()(uint32_t i) const { return b.at(i); }
};
struct Table {
    std::vector<int16_t> t;
    int operator()(int k) const { return t.at((size_t)k); }
    void set(int k, int v) { t.at((size_t)k) = (int16_t)v; }
};

// e* of docs/semantics.md "Alignments" for pattern P at text position g, or -1 above K
static int plainDP(const std::vector<uint8_t>& T, const std::vector<uint8_t>& P, uint32_t g, int K, bool edit) {
    const int m = (int)P.size(), cap = edit ? m + K : m, inf = 1 << 20;
    int JM = 0;
    while (JM < cap && g + JM < T.size() && T[g + JM] != 0) ++JM;
    std::vector<std::vector<int>> D(m + 1, std::vector<int>(JM + 1, inf));
    D[0][0] = 0;
    for (int i = 1; i <= m; ++i)
        for (int j = 0; j <= JM; ++j) {
            int v = inf;
            if (j > 0) v = std::min(v, D[i - 1][j - 1] + (P[i - 1] == T[g + j - 1] ? 0 : 1));
            if (edit) v = std::min(v, D[i - 1][j] + 1);
            if (edit && j > 0 && i < m) v = std::min(v, D[i][j - 1] + 1);
            D[i][j] = std::min(v, inf);
        }
    int best = inf;
    for (int j = 0; j <= JM; ++j) best = std::min(best, D[m][j]);
    return best <= K ? best : -1;
}

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rngState ^= rngState << 13;
    rngState ^= rngState >> 7;
    rngState ^= rngState << 17;
    return (uint32_t)((rngState >> 11) % n);
}

static void tables() {
    for (int round = 0; round < 400; ++round) {
        // two records of a small alphabet (so that placements exist) with a '$' after each; the pattern is a
        // piece of the text with a few edits
        const uint32_t sigma = 2 + rnd(3);
        std::vector<uint8_t> T;
        for (int r = 0; r < 2; ++r) {
            for (uint32_t i = 0, n = 20 + rnd(80); i < n; ++i) T.push_back((uint8_t)(1 + rnd(sigma)));
            T.push_back(0);
        }
        const uint32_t m = 1 + rnd(round % 4 == 0 ? 70 : 24);
        const uint32_t from = rnd((uint32_t)T.size());
        std::vector<uint8_t> P;
        for (uint32_t i = 0; P.size() < m; ++i) {
            const uint8_t c = from + i < T.size() && T[from + i] ? T[from + i] : (uint8_t)(1 + rnd(sigma));
            const uint32_t what = rnd(12);
            if (what == 0) P.push_back((uint8_t)(1 + rnd(sigma)));                       // X (or =)
            else if (what == 1) { P.push_back((uint8_t)(1 + rnd(sigma))); --i; }        // I
            else if (what != 2) P.push_back(c);                                          // (2: D)
        }
        Blocks text(T), pat(P);
        for (int e = 0; e < 2; ++e) {
            const bool edit = e != 0;
            for (uint32_t g = from > 4 ? from - 4 : 0; g < std::min<uint32_t>(from + 5, (uint32_t)T.size()); ++g) {
                const int truth = plainDP(T, P, g, (int)kAlignMaxErr, edit);
                for (uint32_t K = 0; K <= kAlignMaxErr; ++K) {
                    Table L{std::vector<int16_t>((K + 1) * (2 * K + 1), (int16_t)-7)};
                    const int got = alignTable(pat, text, g, m, K, edit, L);
                    const int want = truth >= 0 && truth <= (int)K ? truth : -1;
                    CHECK(got == want);
                    CHECK(got == plainDP(T, P, g, (int)K, edit));
                    // alignOne is the table and the walk: the same e*, and as many edits as that
                    Table L2{std::vector<int16_t>((K + 1) * (2 * K + 1), (int16_t)-7)};
                    uint32_t err, refLen;
                    uint64_t lo, hi;
                    alignOne(pat, text, g, m, K, edit, L2, err, refLen, lo, hi);
                    CHECK((got < 0) == (err == kAlignNone));
                    if (got >= 0) {
                        CHECK(err == (uint32_t)got);
                        int edits = 0, ins = 0, del = 0;
                        for (int s = 0; s < 8; ++s) {
                            const uint32_t v = (uint32_t)((s < 4 ? lo >> (16 * s) : hi >> (16 * (s - 4))) & 0xFFFFu);
                            if (v & 3u) ++edits;
                            ins += (v & 3u) == 2;
                            del += (v & 3u) == 3;
                        }
                        CHECK(edits == got && refLen == m - (uint32_t)ins + (uint32_t)del);
                        // ... and alignTrace over the table that alignTable left gives that record
                        uint32_t err3 = kAlignNone, refLen3 = 0;
                        uint64_t lo3 = 0, hi3 = 0;
                        alignTrace(pat, text, g, m, K, edit, L, got, err3, refLen3, lo3, hi3);
                        CHECK(err3 == err && refLen3 == refLen && lo3 == lo && hi3 == hi);
                    }
                }
            }
        }
    }
}

int main() {
    windows();
    anchorTest();
    order();
    tables();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
