// fm_step.h — one node of the FM phase's DFS (search_fm.hip, kSearchFM),
// written once for a lane of the kernel and for host code: the scheme entry,
// the pattern symbol, the two Occ lines' rank parts and the stack come through
// arguments or accessors, so the same text compiles with a plain C++ compiler
// and runs under the host sanitizers (tests/fm_step_check.cpp).
// docs/semantics.md (policy P0) says what the DFS computes; oracle/oracle.cpp
// (Searcher::visit) is its CPU restatement.
//
// A step has two halves around the fetch of the node's Occ lines, which is
// the caller's (the kernel fetches them pair-cooperatively; the step does not
// assume how they arrived):
//   fmDecode   the node, its scheme entry and pattern symbol -> which children
//              are allowed and which lines (A at lo, B at hi) they need;
//   fmExpand   the lines' rank parts -> the children, pushed match child first
//              and error children above it; one error child stays in registers.
// So a stack holds at most the siblings of the error edges on the current
// path: fmStackCap entries, independent of the pattern length.
// Before either half a node may leave the DFS: as a leaf (fmIsLeaf, fmHit) or,
// once its interval is small, as one text task per row (fmConverts,
// taskRecord), which the text phase finishes against the text (text_step.h).
#pragma once
#include <cstdint>

#include "fm_layout.h"

#ifndef SAHARA_HD  // as align_core.h
#if defined(__HIPCC__)
#define SAHARA_HD __host__ __device__ __forceinline__
#else
#define SAHARA_HD inline
#endif
#endif
// full unrolling of the loops over symbols keeps their arrays in registers on
// the device; a host compiler does not know the pragma
#if defined(__HIPCC__)
#define SAHARA_UNROLL _Pragma("unroll")
#else
#define SAHARA_UNROLL
#endif

namespace sahara {

// Four words: a DFS node (fm_layout.h: x = lb, y = lbRev, z = len, w = meta),
// a hit record or a task record; a uint4 on the device.
struct FmNode {
    uint32_t x, y, z, w;
    SAHARA_HD uint32_t pos() const { return w & 0xFFFFu; }
    SAHARA_HD uint32_t e() const { return (w >> 16) & 0xFu; }
    SAHARA_HD uint32_t lastL() const { return (w >> 20) & 3u; }
    SAHARA_HD uint32_t lastR() const { return (w >> 22) & 3u; }
};

// the entries a lane's DFS stack can hold
SAHARA_HD uint32_t fmStackCap(uint32_t maxErr, uint32_t sigma) { return (maxErr > 1u ? maxErr : 1u) * (2u * sigma - 2u) + 2u; }

// ---- leaves and conversion to text tasks
SAHARA_HD bool fmIsLeaf(const FmNode& n, uint32_t m) { return n.pos() == m; }
// the hit record of a leaf: (qid, lb, len, e)
SAHARA_HD FmNode fmHit(uint32_t pid, const FmNode& n) { return {pid, n.x, n.z, n.e()}; }
// a node of at most `split` rows becomes one text task per row
SAHARA_HD bool fmConverts(const FmNode& n, uint32_t split) { return n.z <= split; }
SAHARA_HD uint32_t fmTextLen(const FmNode& n) { return n.pos() + metaDelta(n.w) - 16u; }  // |t|

// The text-task record: x = an SA row of the node's interval, or (hasPos) the
// text position itself; y = |t| (| kTaskPos); z = pattern; w = the node's meta
// (pos, e, sides) | search << 24. |t| = 0 marks an unused reserved slot.
constexpr uint32_t kTaskPos = 0x80000000u;
struct TextTask {
    uint32_t x, tlen, pid, search, meta;
    bool hasPos;
};
SAHARA_HD FmNode taskRecord(uint32_t x, bool hasPos, const FmNode& n, uint32_t pid, uint32_t search) {
    return {x, fmTextLen(n) | (hasPos ? kTaskPos : 0u), pid, (n.w & 0x00FFFFFFu) | (search << 24)};
}
SAHARA_HD TextTask taskOf(const FmNode& r) {
    return {r.x, r.y & 0xFFFFu, r.z, r.w >> 24, r.w & 0x00FFFFFFu, (r.y & kTaskPos) != 0u};
}

// ---- first half: what the node may do at its position
struct FmDecode {
    uint32_t pos, e, lastL, lastR, cq;
    bool right, matchOK, misOK, delOK, insOK;
    uint32_t lo, hi;    // the interval on the extension side's BWT
    bool needA, needB;  // the line of lo is ranked; hi lies on another line
};
// pattern position that a scheme entry (packScheme) compares
SAHARA_HD uint32_t schemeQ(uint32_t se) { return se & 0xFFFFu; }

// (`live`: the lane holds a node; otherwise no line is needed and the rest is unused)
template <bool EDIT>
SAHARA_HD FmDecode fmDecode(FmNode cur, uint32_t se, uint32_t cq, bool live) {
    FmDecode d;
    d.pos = cur.pos();
    d.e = cur.e();
    d.lastL = cur.lastL();
    d.lastR = cur.lastR();
    d.cq = cq;
    const uint32_t lb = (se >> 16) & 0xFu, ub = (se >> 20) & 0xFu;
    d.right = (se >> 24) & 1u;
    const uint32_t side = d.right ? d.lastR : d.lastL;
    d.matchOK = lb <= d.e && d.e <= ub;
    d.misOK = lb <= d.e + 1 && d.e + 1 <= ub;
    d.delOK = EDIT && d.pos > 0 && d.e + 1 <= ub && side != OP_I;
    d.insOK = EDIT && d.misOK && side != OP_D;
    d.lo = d.right ? cur.y : cur.x;
    d.hi = d.lo + cur.z;
    d.needA = live && (d.matchOK || d.misOK || d.delOK);
    d.needB = d.needA && (d.hi >> 6) != (d.lo >> 6);
    return d;
}

// kind: 0 = match (M), 1 = substitution (S), 2 = deletion (D), 3 = insertion (I)
SAHARA_HD uint32_t childMeta(uint32_t pos, uint32_t e, uint32_t lastL, uint32_t lastR, bool right, uint32_t dl,
                             uint32_t kind) {
    const uint32_t op = kind == 2 ? OP_D : (kind == 3 ? OP_I : OP_MS);
    const uint32_t npos = kind == 2 ? pos : pos + 1u;
    const uint32_t ne = kind == 0 ? e : e + 1u;
    const uint32_t nl = pos == 0 ? op : (right ? lastL : op);
    const uint32_t nr = pos == 0 ? op : (right ? op : lastR);
    const uint32_t nd = dl + (kind == 2 ? 1u : 0u) - (kind == 3 ? 1u : 0u);
    return npos | (ne << 16) | (nl << 20) | (nr << 22) | (nd << 25);
}

// Children of one DFS node under policy P0 (docs/semantics.md), with the
// stack discipline described at the top. `occ[c]` says whether the child of
// symbol c exists; `mk(c, kind)` builds it. Returns whether a child is kept
// in registers (through `next`).
template <int SIGMA, typename Node, typename MkChild, typename Push>
SAHARA_HD bool expandChildren(const uint32_t occ[SIGMA], uint32_t cq, bool matchOK, bool misOK, bool delOK, bool insOK,
                              const Node& insChild, MkChild mk, Push push, Node& next) {
    uint32_t nErr = insOK ? 1u : 0u;
    bool hasM = false;
SAHARA_UNROLL
    for (int c = 1; c < SIGMA; ++c) {
        if (occ[c]) {
            if ((uint32_t)c == cq) hasM = matchOK;
            else nErr += misOK ? 1u : 0u;
            nErr += delOK ? 1u : 0u;
        }
    }
    bool kept = false;
    auto emit = [&](const Node& v) {
        if (!kept) { next = v; kept = true; }
        else push(v);
    };
    if (hasM && nErr) push(mk((int)cq, 0));  // match child below all its error siblings
    if (insOK) emit(insChild);
SAHARA_UNROLL
    for (int c = 1; c < SIGMA; ++c) {
        if (occ[c]) {
            if ((uint32_t)c != cq && misOK) emit(mk(c, 1));
            if (delOK) emit(mk(c, 2));
        }
    }
    if (!kept && hasM) { next = mk((int)cq, 0); kept = true; }
    return kept;
}

// ---- second half: rank all symbols at lo and hi from the rank parts of their
// lines (cnt[5], plane[3] of OccLine; line B is read only when d.needB: lo and
// hi share line A otherwise), update both sides' intervals, and expand the
// children: C is the index's C array (C[c] = symbols smaller than c),
// `push(node)` stacks a child, `next` is the one the lane continues with.
// Returns whether there is one.
template <int SIGMA, typename Push>
SAHARA_HD bool fmExpand(FmNode cur, const FmDecode& d, const uint32_t cntA[5], const uint64_t planeA[3],
                        const uint32_t cntB[5], const uint64_t planeB[3], const uint32_t* C, Push push, FmNode& next) {
    // child c = (fx[c], fy[c], occ[c]): forward / reverse lower bounds
    uint32_t occ[SIGMA], fx[SIGMA], fy[SIGMA];
SAHARA_UNROLL
    for (int c = 0; c < SIGMA; ++c) occ[c] = fx[c] = fy[c] = 0;
    if (d.needA) {
        uint32_t cb[5];
        uint64_t pb[3];
SAHARA_UNROLL
        for (int i = 0; i < 5; ++i) cb[i] = d.needB ? cntB[i] : cntA[i];
SAHARA_UNROLL
        for (int i = 0; i < 3; ++i) pb[i] = d.needB ? planeB[i] : planeA[i];
        const uint64_t ml = lowMask(d.lo & 63u), mh = lowMask(d.hi & 63u);
        uint32_t sum = 0, base[SIGMA];
SAHARA_UNROLL
        for (int c = 1; c < SIGMA; ++c) {
            const uint32_t rl = cntA[c - 1] + (uint32_t)__builtin_popcountll(symMask(planeA, c) & ml);
            const uint32_t rh = cb[c - 1] + (uint32_t)__builtin_popcountll(symMask(pb, c) & mh);
            occ[c] = rh - rl;
            base[c] = C[c] + rl;
            sum += occ[c];
        }
        // bidirectional update: the other side moves by the occurrences
        // of the smaller symbols, '$' first
        uint32_t acc = (d.right ? cur.x : cur.y) + (cur.z - sum);
SAHARA_UNROLL
        for (int c = 1; c < SIGMA; ++c) {
            fx[c] = d.right ? acc : base[c];
            fy[c] = d.right ? base[c] : acc;
            acc += occ[c];
        }
    }
    const uint32_t dl = metaDelta(cur.w);
    auto mk = [&](int c, uint32_t kind) -> FmNode {
        uint32_t f = 0, g = 0, o = 0;
SAHARA_UNROLL
        for (int s = 1; s < SIGMA; ++s)
            if (s == c) { f = fx[s]; g = fy[s]; o = occ[s]; }
        return {f, g, o, childMeta(d.pos, d.e, d.lastL, d.lastR, d.right, dl, kind)};
    };
    const FmNode ins = {cur.x, cur.y, cur.z, childMeta(d.pos, d.e, d.lastL, d.lastR, d.right, dl, 3)};
    next = {0, 0, 0, 0};
    return expandChildren<SIGMA>(occ, d.cq, d.matchOK, d.misOK, d.delOK, d.insOK, ins, mk, push, next);
}

}  // namespace sahara
