// align_core.h — the alignment of one located hit (docs/semantics.md,
// "Alignments"), written once for the kernel (align.hip) and for host code:
// pattern and text come through accessors that return one 3-bit-plane block
// of 32 symbols (device_index.h), the table through an accessor of small
// integers, so the same text compiles for a lane and for a host thread.
//
// The form: furthest-reaching rows. L[e][d] = the largest i with
// D[i][i + d] <= e (kNoCell: no cell of diagonal d = j - i costs <= e), for
// e <= K and |d| <= K (edit off: d = 0 only). D is non-decreasing along a
// diagonal, so D[i][j] = the least e with L[e][j - i] >= i, which is all the
// backward walk needs. Row 0 of D is special in both directions: (0, j > 0)
// is no cell (a D can never be first), so a diagonal d > 0 starts at row 1;
// row m takes no D (never last), so a D leaves a diagonal at row m - 1 at the
// latest, whatever that diagonal's furthest row is.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SAHARA_HD __host__ __device__ __forceinline__
#else
#define SAHARA_HD inline
#endif

namespace sahara {

struct Planes3 { uint32_t b0, b1, b2; };

constexpr int kNoCell = -1;
constexpr uint32_t kAlignNone = 0xFFFFFFFFu;
constexpr uint32_t kAlignMaxErr = 8;
constexpr uint32_t kAlignMaxLen = 16383;  // qpos << 2 | kind in 16 bits
constexpr int kAlignInf = 1 << 20;

SAHARA_HD uint32_t alignCtz(uint32_t x) { return x ? (uint32_t)__builtin_ctz(x) : 32u; }
SAHARA_HD uint32_t alignClz(uint32_t x) { return x ? (uint32_t)__builtin_clz(x) : 32u; }
SAHARA_HD uint32_t alignFunnel(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31u));
}
// 32 symbols from symbol `at` of a block array
template <class F>
SAHARA_HD Planes3 alignRead32(F& blocks, uint32_t at) {
    const uint32_t b = at >> 5, sh = at & 31u;
    const Planes3 lo = blocks(b), hi = blocks(b + 1);
    return {alignFunnel(hi.b0, lo.b0, sh), alignFunnel(hi.b1, lo.b1, sh), alignFunnel(hi.b2, lo.b2, sh)};
}

// The table build of one hit: pattern of m symbols (pat(b): its block b,
// b <= ceil(m / 32): the block after the pattern is read and masked), text
// position g (text(b): text block b, zero blocks after the text), bound
// K <= kAlignMaxErr. L holds (K + 1) * (2 K + 1) entries; rows 0 .. e* of it
// are filled. Returns e*, or -1 if no alignment costs K or less. For K below
// the true e* the answer is -1, for any K at or above it the same e*: a cell
// of cost e lies within |d| <= e and within m + e text symbols. (The mate
// rescue's scan, rescue.hip, calls this alone, with a falling bound.)
template <class PF, class TF, class LT>
SAHARA_HD int alignTable(PF& pat, TF& text, uint32_t g, uint32_t m, uint32_t K, bool edit, LT& L) {
    // the window: text symbols up to the first '$' (all planes 0: the pad after the text too)
    const uint32_t cap = edit ? m + K : m;
    uint32_t JM = 0;
    for (;;) {
        const Planes3 t = alignRead32(text, g + JM);
        const uint32_t n = alignCtz(~(t.b0 | t.b1 | t.b2));
        JM += n;
        if (n < 32u || JM >= cap) break;
    }
    if (JM > cap) JM = cap;
    const int B = edit ? (int)K : 0, W = 2 * B + 1;
    const int M = (int)m, J = (int)JM;
    // matches from cell (i, i + d) on, along the diagonal
    auto slide = [&](int i, int d) {
        int j = i + d;
        int lim = M - i < J - j ? M - i : J - j;
        while (lim > 0) {
            const Planes3 p = alignRead32(pat, (uint32_t)i), t = alignRead32(text, g + (uint32_t)j);
            const int n = (int)alignCtz((p.b0 ^ t.b0) | (p.b1 ^ t.b1) | (p.b2 ^ t.b2));
            const int step = n < lim ? n : lim;
            i += step;
            j += step;
            lim -= step;
            if (n < 32) break;
        }
        return i;
    };
    int eStar = -1;
    for (int e = 0; e <= (int)K && eStar < 0; ++e) {
        for (int d = -B; d <= B; ++d) {
            int best = kNoCell;
            if (e == 0) {
                if (d == 0) best = 0;
            } else {
                const int up = L((e - 1) * W + d + B);
                best = up;                                              // costs <= e - 1
                if (up >= 0 && up < M && up + d + 1 <= J && up + 1 > best) best = up + 1;  // X
                if (d + 1 <= B) {                                       // I: (i - 1, j) -> (i, j)
                    const int r = L((e - 1) * W + d + 1 + B);
                    const int i = r < M - 1 ? r : M - 1;
                    if (r >= 0 && i >= 0 && i + d + 1 >= 0 && (i > 0 || d + 1 == 0) && i + 1 > best) best = i + 1;
                }
                if (d - 1 >= -B) {                                      // D: (i, j - 1) -> (i, j), 0 < i < m
                    const int r = L((e - 1) * W + d - 1 + B);
                    const int i = r < M - 1 ? r : M - 1;
                    if (r >= 0 && i >= 1 && i + d - 1 >= 0 && i + d <= J && i > best) best = i;
                }
            }
            if (best >= 0) best = slide(best, d);
            L.set(e * W + d + B, best);
            if (best == M) eStar = e;
        }
    }
    return eStar;
}

// The backward walk over a table that alignTable built for the same m, K and
// edit and that reached eStar >= 0: refLen and the edits, err = eStar (the
// record stays NONE should the walk find no predecessor, which a table built
// above never causes).
template <class PF, class TF, class LT>
SAHARA_HD void alignTrace(PF& pat, TF& text, uint32_t g, uint32_t m, uint32_t K, bool edit, LT& L, int eStar,
                          uint32_t& err, uint32_t& refLen, uint64_t& edLo, uint64_t& edHi) {
    const int B = edit ? (int)K : 0, W = 2 * B + 1;
    const int M = (int)m;
    // ref_len: the end closest to m, ties to the smaller j
    int dEnd = 0;
    for (int t = 0; t <= B; ++t) {
        if (L(eStar * W - t + B) == M) { dEnd = -t; break; }
        if (L(eStar * W + t + B) == M) { dEnd = t; break; }
    }
    auto cost = [&](int i, int j) {
        if (j < 0 || i < 0) return kAlignInf;
        if (i == 0) return j == 0 ? 0 : kAlignInf;
        const int d = j - i;
        if (d < -B || d > B) return kAlignInf;
        for (int e = 0; e <= eStar; ++e)
            if (L(e * W + d + B) >= i) return e;
        return kAlignInf;
    };
    int i = M, j = M + dEnd, c = eStar;
    auto emit = [&](int qpos, int kind) {
        const uint64_t v = (uint64_t)(((uint32_t)qpos << 2) | (uint32_t)kind);
        const int s = c - 1;
        if (s < 4) edLo |= v << (16 * s);
        else edHi |= v << (16 * (s - 4));
        --c;
    };
    while (i > 0 || j > 0) {
        bool lastEq = false;
        if (i > 0 && j > 0) {
            // matches backwards: a match's diagonal predecessor always has the cell's cost
            const int n = i < j ? (i < 32 ? i : 32) : (j < 32 ? j : 32);
            const Planes3 p = alignRead32(pat, (uint32_t)(i - n)), t = alignRead32(text, g + (uint32_t)(j - n));
            const uint32_t eq = ~((p.b0 ^ t.b0) | (p.b1 ^ t.b1) | (p.b2 ^ t.b2));
            int run = (int)alignClz(~(eq << (32 - n)));
            if (run > n) run = n;
            lastEq = run > 0;
            if (j > i && run > i - 1) run = i - 1;  // (0, j > 0) is no cell
            if (run > 0) {
                i -= run;
                j -= run;
                continue;
            }
        }
        if (i > 0 && j > 0) {
            const int sub = lastEq ? 0 : 1;
            if (cost(i - 1, j - 1) + sub == c) {
                if (sub) emit(i - 1, 1);
                --i;
                --j;
                continue;
            }
        }
        if (edit && i > 0 && cost(i - 1, j) + 1 == c) {
            emit(i - 1, 2);
            --i;
            continue;
        }
        if (edit && i > 0 && i < M && j > 0 && cost(i, j - 1) + 1 == c) {
            emit(i, 3);
            --j;
            continue;
        }
        return;  // unreachable for a table built above; the record stays NONE
    }
    err = (uint32_t)eStar;
    refLen = (uint32_t)(M + dEnd);
}

// One hit: the table, then the walk. Result: err (kAlignNone: no alignment
// within K), refLen, and the err edits, 16 bits each, in pattern order: edit
// s in bits 16 (s % 4) of edLo (s < 4) or edHi.
template <class PF, class TF, class LT>
SAHARA_HD void alignOne(PF& pat, TF& text, uint32_t g, uint32_t m, uint32_t K, bool edit, LT& L, uint32_t& err,
                        uint32_t& refLen, uint64_t& edLo, uint64_t& edHi) {
    err = kAlignNone;
    refLen = 0;
    edLo = edHi = 0;
    const int eStar = alignTable(pat, text, g, m, K, edit, L);
    if (eStar < 0) return;
    alignTrace(pat, text, g, m, K, edit, L, eStar, err, refLen, edLo, edHi);
}

}  // namespace sahara
