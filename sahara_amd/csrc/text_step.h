// text_step.h — the micro-step of the text phase's DFS (search_text.hip,
// kSearchTextBatch), written once for a lane of the kernel and for host code:
// the table row, the pattern, the window and the stack come through
// accessors, so the same text compiles with a plain C++ compiler and runs
// under the host sanitizers (tests/text_step_check.cpp). tests/text_model.py
// is the readable statement of what a step does; docs/semantics.md (policy
// P0) of what the DFS computes.
//
// A lane's state is one DFS node (TextNode) and a stack of at most 2k + 2 of
// them. A node with e == u[pos] has no error child in the forced run of
// positions that follows it (TextRow::run), so it matches up to kRun symbols
// at once; a node whose error children are forced walks up to kChain
// positions of its match chain and checks every error child's forced run on
// the way: the DFS visits the same nodes, one micro-step per run or chain.
#pragma once
#include <cstddef>
#include <cstdint>

#include <algorithm>
#include <vector>

#include "fm_layout.h"

#ifndef SAHARA_HD  // as align_core.h
#if defined(__HIPCC__)
#define SAHARA_HD __host__ __device__ __forceinline__
#else
#define SAHARA_HD inline
#endif
#endif

namespace sahara {

// ---- runs of symbols as bit masks: bit j = chain symbol j. Symbols come as
// 3 bit planes (device_index.h), so the per-symbol equality of 32 symbols is
// three word xors.
constexpr uint32_t kRun = 32;  // symbols per micro-step run (a forced node's match budget)
constexpr uint32_t kRunMask = 0xFFFFFFFFu;
// chain positions per micro-step of a node whose error children are forced:
// the forced-run check of an error child at chain node i reads symbols
// i .. i + 7 of the 32 (kChain + 7 <= kRun)
constexpr uint32_t kChain = 25;
static_assert(kChain + 7u <= kRun && kRun == 32u, "a run is one word per plane");

SAHARA_HD uint32_t textMin(uint32_t a, uint32_t b) { return a < b ? a : b; }
SAHARA_HD uint32_t textMax(uint32_t a, uint32_t b) { return a > b ? a : b; }
SAHARA_HD uint32_t textCtz(uint32_t x) { return x ? (uint32_t)__builtin_ctz(x) : kRun; }  // all-zero word: kRun
SAHARA_HD uint32_t textCtz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }         // x != 0
SAHARA_HD uint32_t textPopc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

SAHARA_HD uint32_t onesR(uint32_t n) {  // symbols [0, n), capped at kRun
    return n >= kRun ? kRunMask : (1u << n) - 1u;
}
SAHARA_HD uint32_t beyondR(uint32_t n) { return kRunMask & ~onesR(n); }  // symbols >= n
// bit j set iff bits j .. j+6 are all set (7 consecutive matches from j)
SAHARA_HD uint32_t run7(uint32_t m) {
    const uint32_t m2 = m & (m >> 1), m4 = m2 & (m2 >> 2);
    return m4 & (m2 >> 4) & (m >> 6);
}
struct Planes { uint32_t b0, b1, b2; };
SAHARA_HD uint32_t eqm(const Planes& p, const Planes& t) {
    return ~((p.b0 ^ t.b0) | (p.b1 ^ t.b1) | (p.b2 ^ t.b2));
}
SAHARA_HD Planes shr1(const Planes& p) { return {p.b0 >> 1, p.b1 >> 1, p.b2 >> 1}; }
SAHARA_HD Planes shr2(const Planes& p) { return {p.b0 >> 2, p.b1 >> 2, p.b2 >> 2}; }

// One DFS node: x = window offsets xo | yo << 16 of the text t matched so far
// (the span [xo, yo)), y = pos | e << 16 | lastL << 20 | lastR << 22 (pos in
// 16 bits, e in 4: e <= 15; the last operation on either side, OP_*).
struct TextNode {
    uint32_t x, y;
    SAHARA_HD uint32_t xo() const { return x & 0xFFFFu; }
    SAHARA_HD uint32_t yo() const { return x >> 16; }
    SAHARA_HD uint32_t pos() const { return y & 0xFFFFu; }
    SAHARA_HD uint32_t e() const { return (y >> 16) & 0xFu; }
    SAHARA_HD uint32_t lastL() const { return (y >> 20) & 3u; }
    SAHARA_HD uint32_t lastR() const { return (y >> 22) & 3u; }
};
// span [xo, yo) with the given meta word (a task record's: pos | e << 16 | sides)
SAHARA_HD TextNode textNode(uint32_t xo, uint32_t yo, uint32_t meta) { return {xo | (yo << 16), meta}; }

// One row of the text-phase table (textTable below), two words per (search, pos):
//   x = packScheme(pi, l, u, right) | run << 25 — run = number of consecutive
//       positions from pos (<= 127) on the same side with u == u[pos] and
//       l <= u[pos]: a node at pos with e == u[pos] has no error child
//       anywhere in that run, so the DFS is a forced chain of matches through it;
//   y = a | b << 12 | same << 24 — pattern positions [a, b) covered before
//       step pos; `same` (<= run) positions from pos share pos's l as well,
//       so a chain of matches through them branches the same way at each.
struct TextRow {
    uint32_t x, y;
    SAHARA_HD uint32_t q() const { return x & 0xFFFFu; }
    SAHARA_HD uint32_t lb() const { return (x >> 16) & 0xFu; }
    SAHARA_HD uint32_t ub() const { return (x >> 20) & 0xFu; }
    SAHARA_HD bool right() const { return (x >> 24) & 1u; }
    SAHARA_HD uint32_t run() const { return x >> 25; }
    SAHARA_HD uint32_t coverBegin() const { return y & 0xFFFu; }
    SAHARA_HD uint32_t coverEnd() const { return (y >> 12) & 0xFFFu; }
    SAHARA_HD uint32_t same() const { return (y >> 24) & 0x7Fu; }
};

// The table of ns searches over m positions from the scheme and its packed
// form (packScheme per position): 2 words per row, as TextRow reads them.
inline void textTable(const uint32_t* pi, const uint32_t* l, const uint32_t* u, uint32_t ns, uint32_t m,
                      const std::vector<uint32_t>& packed, std::vector<uint32_t>& out) {
    out.assign((size_t)ns * m * 2, 0);
    for (uint32_t s = 0; s < ns; ++s) {
        const uint32_t* P = pi + (size_t)s * m;
        const uint32_t* L = l + (size_t)s * m;
        const uint32_t* U = u + (size_t)s * m;
        const uint32_t* Q = packed.data() + (size_t)s * m;
        uint32_t a = P[0], b = P[0];
        for (uint32_t p = 0; p < m; ++p) {
            const uint32_t right = (Q[p] >> 24) & 1u;
            uint32_t run = 1, same = 1;
            while (run < 127 && p + run < m && ((Q[p + run] >> 24) & 1u) == right && U[p + run] == U[p] &&
                   L[p + run] <= U[p])
                ++run;
            while (same < run && L[p + same] == L[p]) ++same;
            out[((size_t)s * m + p) * 2] = Q[p] | (run << 25);
            out[((size_t)s * m + p) * 2 + 1] = a | (b << 12) | (same << 24);
            a = std::min(a, P[p]);
            b = std::max(b, P[p] + 1);
        }
    }
}

// What one micro-step leaves behind.
struct TextStepResult {
    TextNode cur;        // the node the lane continues with (if have)
    uint32_t sp;         // stack entries afterwards
    bool have;           // the lane still holds a node
    bool leaf;           // the node was a leaf (pos == m): a hit at window offset leafStart with leafE errors
    uint32_t leafStart, leafE;
    bool bad;            // the stack bound would have been violated (cannot happen: flagged, not handled)
    uint32_t nodes, compares, steps;  // count mode: chain nodes expanded, forced-run comparisons, steps of a node
};

// One micro-step of the node `cur` (`live`: the lane holds one; otherwise
// nothing changes) with sp entries on the lane's stack of stackCap, for a
// pattern of m symbols and a window of winLen:
//   row(p)            the TextRow of position p < m of the node's search
//   pat(o, fwd)       32 pattern symbols in chain order as Planes: right from
//   win(o, fwd)       offset o (fwd), or left ending at o - 1, bit j = symbol
//                     o - 1 - j. Symbols outside the pattern are arbitrary
//                     (never used); those outside the window are masked here.
//   stackPut(d, node) writes stack entry d < stackCap
// Straight-line code but for the loop over the surviving error children, so
// the lanes of a wave stay converged.
template <bool EDIT, typename Row, typename Pat, typename Win, typename Put>
SAHARA_HD TextStepResult textStep(const TextNode& cur, uint32_t sp, bool live, uint32_t stackCap, uint32_t m,
                                  uint32_t winLen, Row row, Pat pat, Win win, Put stackPut) {
    const uint32_t pos = cur.pos();
    const uint32_t xo = cur.xo(), yo = cur.yo();
    const uint32_t e = cur.e();
    const uint32_t lastL = cur.lastL(), lastR = cur.lastR();
    const TextRow tab = row(textMin(pos, m - 1u));
    const uint32_t q0 = tab.q(), lb0 = tab.lb(), ub0 = tab.ub();
    const bool r0 = tab.right();
    const uint32_t run0 = tab.run(), same0 = tab.same();

    // ---- pattern symbols from pi[pos] in this step's direction and the text
    // symbols beyond the span on that side, both in chain order (symbol j of
    // the chain in bit j); text past the window edge or before its start is
    // masked by `avail` and never matches. One read each at a side-dependent
    // offset (a left run ends at the position and is bit-reversed), so the
    // lanes of both sides share it
    const Planes PC = pat(r0 ? q0 : q0 + 1u, r0);
    const Planes TC = win(r0 ? yo : xo, r0);
    const uint32_t avail = r0 ? (winLen > yo ? winLen - yo : 0u) : xo;
    const uint32_t VT = onesR(avail);
    const uint32_t E0 = eqm(PC, TC) & VT;                 // p_j == t_j     (M chain, S runs)
    const uint32_t ED = eqm(PC, shr1(TC)) & (VT >> 1);    // p_j == t_{j+1} (D runs)
    const uint32_t EI = eqm(shr1(PC), TC) & VT;           // p_{j+1} == t_j (I runs)
    const uint32_t TZ = (TC.b0 | TC.b1 | TC.b2) & VT;     // t_j is a symbol (not '$' / edge)

    const bool atLeaf = live && pos == m;
    const bool node = live && pos < m;
    const bool forced = e == ub0;          // no error child here or in the rest of the run
    const bool kidsF = e + 1u == ub0;      // the error children are forced nodes
    const bool mOK = lb0 <= e && e <= ub0;
    const bool misOK = lb0 <= e + 1u && e + 1u <= ub0;
    const uint32_t side = r0 ? lastR : lastL;
    // chain budget: a forced node matches up to kRun symbols; a node whose
    // error children are forced walks up to kChain positions of its match
    // chain (same direction, l and u), checking every error child's forced
    // run on the way; any other node is expanded alone
    const uint32_t B = forced ? textMin(run0, kRun)
                              : (kidsF ? textMax(1u, textMin(textMin(same0, run0 - 1u), kChain)) : 1u);
    const uint32_t L = mOK ? textMin(B, textCtz(~E0 & kRunMask)) : 0u;

    // ---- error children of the chain nodes i < NN (node L = the mismatch)
    const uint32_t NN = L < B ? L + 1u : B;
    const uint32_t nodesM = node && !forced ? onesR(NN) : 0u;  // leaves / idle lanes: none
    const uint32_t first = 1u;  // chain node 0 (= this node)
    uint32_t Dm = EDIT ? (nodesM & TZ) : 0u;
    if (pos == 0u || side == OP_I) Dm &= ~first;
    uint32_t Im = EDIT && misOK ? nodesM : 0u;
    if (side == OP_D) Im &= ~first;
    // S at the first mismatch (not where M is merely disallowed: l > e)
    bool Sx = node && !forced && L < B && misOK && ((TZ & ~E0) >> L) & 1u;
    // forced runs: a child at e + 1 = u is forced for the rest of the run,
    // and survives only if min(7, rest of the run) symbols match on its
    // diagonal (positions past the run count as matches): R7x bit j =
    // that check for a run starting at chain position j on diagonal x
    const uint32_t bR = beyondR(run0), bR1 = beyondR(run0 - 1u);
    const uint32_t R7E0 = run7(E0 | bR), R7ED = run7(ED | bR), R7EI = run7(EI | bR1);
    if (kidsF) {
        // D at i: p[i..] vs t[i+1..]; I at i: p[i+1..] vs t[i..]; S at L: p[L+1..] vs t[L+1..]
        Dm &= R7ED;
        Im &= R7EI;
        Sx = Sx && ((R7E0 >> (L + 1u)) & 1u);
    }
    if (EDIT && node && e + 2u == ub0) {
        // A node expanded alone whose error children are chain nodes: keep
        // only the children whose subtree outlives their own first step. A
        // child does if its match chain leaves the run or the 32 symbols read
        // (chain length > kRun - 9), or one of its own error children
        // (forced) passes the check above on its diagonal; no I right after
        // D, no D right after I (policy P0). tests/text_model.py holds this
        // to the plain DFS.
        const uint32_t ED2 = eqm(PC, shr2(TC)) & (VT >> 2);   // p_j == t_{j+2}
        const uint32_t EI2 = eqm(shr2(PC), TC) & VT;          // p_{j+2} == t_j
        const uint32_t bR2 = run0 >= 2u ? beyondR(run0 - 2u) : kRunMask;
        const uint32_t R7ED2 = run7(ED2 | bR), R7EI2 = run7(EI2 | bR2);
        const uint32_t I2after = (R7E0 >> 1) & ~1u;  // bit j: I2 (back to diagonal 0) at chain node j > 0
        constexpr uint32_t kLim = kRun - 9u;
        if (Dm & first) {  // D child: p_j vs t_{j+1}
            const uint32_t LD = textCtz(~ED);  // (bit 31 of ED is never set)
            const bool keep = LD >= run0 || LD > kLim || ((R7ED >> (LD + 1u)) & 1u) ||
                              ((R7ED2 | I2after) & onesR(LD + 1u)) != 0u;
            if (!keep) Dm &= ~first;
        }
        if (Im & first) {  // I child: p_{x+1} vs t_x
            const uint32_t LI = textCtz(~EI);
            const bool keep = LI + 1u >= run0 || LI > kLim || ((R7EI >> (LI + 1u)) & 1u) ||
                              ((I2after | R7EI2) & onesR(LI + 1u)) != 0u;
            if (!keep) Im &= ~first;
        }
        if (Sx) {  // S child at the mismatch L = 0: p_x vs t_x, x >= 1
            const uint32_t LS = textCtz(~E0 & ~1u);
            Sx = LS >= run0 || LS > kLim || ((R7E0 >> (LS + 1u)) & 1u) ||
                 ((R7ED | R7EI) & ~1u & onesR(LS + 1u)) != 0u;
        }
    }
    const bool contM = node && L >= B;  // the match chain continues at pos + B
    uint32_t nSurv = textPopc(Dm) + textPopc(Im) + (Sx ? 1u : 0u);
    // the lane continues with one child and stacks the others: a surviving
    // error child first, the match chain below it
    uint32_t Bc = B;
    // Stack invariant (stackCap = 2k + 2): a node that stacks entries with e
    // errors finds sp <= 2e + 2. One node expanded alone stacks <= 2; a chain
    // may stack more only while the child it continues with (e + 1) still
    // finds sp <= 2(e + 1) + 2.
    if (nSurv && sp + nSurv + (contM ? 1u : 0u) - 1u > 2u * e + 4u) {
        // not enough stack for this chain: expand its first node only
        Bc = 1u;
        Dm &= first;
        Im &= first;
        Sx = Sx && L == 0u;
        nSurv = textPopc(Dm) + textPopc(Im) + (Sx ? 1u : 0u);
    }
    const bool contM1 = node && L >= Bc;

    TextStepResult res;
    // cannot happen (the reserve rule above; tests/text_model.py): flagged, not handled
    res.bad = node && nSurv && sp + nSurv + (contM1 ? 1u : 0u) - 1u > stackCap;

    // ---- children as stack entries (x = span, y = meta). Per step: extending
    // by n symbols adds n << 16 (right) or -n (left) to the span, one mad; a
    // child's side memory is its operation on the extension side (MS once k
    // forced matches follow it), the other side keeps its memory — except at
    // pos 0, where the first operation sets both (for chain node i > 0 that
    // was a match)
    const int extMul = r0 ? 65536 : -1;
    auto extend = [&](uint32_t span, uint32_t n) -> uint32_t { return span + (uint32_t)((int)n * extMul); };
    const uint32_t shMine = r0 ? 22u : 20u, shOther = r0 ? 20u : 22u;
    const uint32_t otherKept = pos ? (r0 ? lastL : lastR) : (uint32_t)OP_MS;
    auto metaAt = [&](uint32_t i, uint32_t op, uint32_t k) -> uint32_t {
        const uint32_t mine = k ? (uint32_t)OP_MS : op;
        const uint32_t other = (pos == 0u && i == 0u) ? op : otherKept;
        return (mine << shMine) | (other << shOther);
    };
    const uint32_t e1 = (e + 1u) << 16;
    // forced matches after an error child whose run starts at chain node ii
    const uint32_t kEnd = kidsF ? run0 : 0u;
    const TextNode cM = {extend(cur.x, Bc), (pos + Bc) | (e << 16) | metaAt(Bc, OP_MS, 0u)};
    res.cur = cur;
    res.sp = sp;
    if (nSurv) {  // the surviving error children; the last one stays in registers
        uint32_t spw = sp;
        TextNode pend = cM;
        bool hasPend = contM1;
        // one loop over all of them — D at chain node i (bit i), I at i (bit
        // 32 + i), S at L (bit 63), in that order — so the wave runs
        // max(nSurv) iterations rather than one loop per kind
        uint64_t sv = (uint64_t)Dm | ((uint64_t)Im << 32) | (Sx ? 1ull << 63 : 0ull);
        while (sv) {
            const uint32_t j = textCtz64(sv);
            sv &= sv - 1ull;
            const bool isS = j == 63u, isD = j < 32u, isI = !isD && !isS;
            const uint32_t i = isS ? L : (j & 31u);
            const uint32_t ii = i + (isD ? 0u : 1u);  // chain node where its forced run starts
            const uint32_t k = ii < kEnd ? textMin(kEnd - ii, 7u) : 0u;
            const uint32_t op = isD ? (uint32_t)OP_D : (isI ? (uint32_t)OP_I : (uint32_t)OP_MS);
            const TextNode v = {extend(cur.x, i + k + (isI ? 0u : 1u)), (pos + ii + k) | e1 | metaAt(i, op, k)};
            if (hasPend) stackPut(textMin(spw++, stackCap - 1u), pend);
            pend = v;
            hasPend = true;
        }
        res.sp = textMin(spw, stackCap);
        res.cur = pend;
    } else if (node && contM1) {
        res.cur = cM;
    }

    res.leaf = atLeaf;
    res.leafStart = xo;
    res.leafE = e;
    res.have = node && (nSurv || contM1);
    res.nodes = forced ? 0u : (node ? NN : 0u);
    res.compares = (node && forced) ? 1u : 0u;
    res.steps = node ? 1u : 0u;
    return res;
}

}  // namespace sahara
