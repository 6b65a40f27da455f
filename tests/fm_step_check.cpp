// The FM kernel's node step (csrc/fm_step.h) run on the host as a DFS — pop,
// leaf or convert, decode, rank and expand, stack — over the cases that
// tests/test_fm_step.py writes from the index model and the oracle. Per case:
//   split = 0      the leaf cursors, their located positions and the node /
//                  rank-node / Occ-line counts must equal the oracle's;
//   split = 1, 4   nodes of at most `split` rows leave as task records, each
//                  decoded again and finished by the text kernel's step
//                  (csrc/text_step.h) with the whole text as its window: FM
//                  leaves and text leaves together must equal the oracle's
//                  located hits as a multiset.
// No push may pass fmStackCap, no text step may set `bad`. Built under the
// address and undefined-behaviour sanitizers.
#include <array>
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../sahara_amd/csrc/fm_step.h"
#include "../sahara_amd/csrc/text_step.h"
#include "planes_host.h"

using namespace sahara;

namespace {

int failures = 0;
void fail(const char* what, long ca, long split) {
    if (++failures <= 20) std::printf("FAIL case %ld split %ld: %s\n", ca, split, what);
}

std::vector<uint32_t> readRow(std::istream& in, size_t n) {
    std::vector<uint32_t> v(n);
    for (auto& x : v) in >> x;
    return v;
}

// one OccLine per 64 BWT rows, and one more so that hi = n has a line
std::vector<OccLine> occLines(const std::vector<uint32_t>& bwt) {
    std::vector<OccLine> L(bwt.size() / 64 + 1);
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t b = 0; b < L.size(); ++b) {
        OccLine& o = L[b];
        o = OccLine{};
        for (uint32_t c = 1; c <= 5; ++c) o.cnt[c - 1] = cnt[c];
        for (size_t j = 0; j < 64 && b * 64 + j < bwt.size(); ++j) {
            const uint32_t s = bwt[b * 64 + j];
            for (int p = 0; p < 3; ++p) o.plane[p] |= (uint64_t)((s >> p) & 1u) << j;
            ++cnt[s];
        }
    }
    return L;
}

using Cursor = std::array<uint64_t, 4>;  // qid, lb, len, e
using Hit = std::array<uint64_t, 3>;     // qid, text position, e
template <class K>
using Multiset = std::map<K, long>;

struct Case {
    uint32_t sigma, edit, k, m, n, ns, npat;
    std::vector<uint32_t> C, sa, pi, l, u, pats, packed, table;
    std::vector<OccLine> occF, occR;
    std::vector<uint32_t> text;
};

struct Tally {
    uint64_t nodes = 0, rankNodes = 0, lines = 0, tasks = 0, multiConversions = 0, insChildren = 0, delChildren = 0;
    uint64_t needB[2] = {0, 0};
};

// A DFS's stack of fmStackCap entries and what leaves it. Its members are
// kept out of line and the drivers below out of templates where they can be:
// under -g and the sanitizers the container code costs seconds per copy.
struct Dfs {
    std::vector<FmNode> stack;
    uint32_t sp = 0;
    bool firstPos = false, right = false;  // of the node being expanded
    Tally& t;
    long ca, split;
    Multiset<Cursor>& leaves;
    std::vector<FmNode>& tasks;
    Dfs(uint32_t cap, Tally& tally, long c, long s, Multiset<Cursor>& lv, std::vector<FmNode>& tk)
        : stack(cap), t(tally), ca(c), split(s), leaves(lv), tasks(tk) {}
    [[gnu::noinline]] void leaf(uint32_t pid, const FmNode& n) {
        const FmNode h = fmHit(pid, n);
        ++leaves[{h.x, h.y, h.z, h.w}];
    }
    [[gnu::noinline]] void convert(uint32_t pid, uint32_t s, const FmNode& n) {
        for (uint32_t j = 0; j < n.z; ++j) tasks.push_back(taskRecord(n.x + j, false, n, pid, s));
        t.tasks += n.z;
        t.multiConversions += n.z >= 2 ? 1 : 0;
    }
    [[gnu::noinline]] bool pop(FmNode& cur) {
        if (sp == 0) return false;
        cur = stack[--sp];
        return true;
    }
    // a child's operation is its memory on the extension side (both sides at the first position)
    [[gnu::noinline]] void note(const FmNode& v) {
        const uint32_t op = firstPos ? v.lastL() : (right ? v.lastR() : v.lastL());
        t.insChildren += op == OP_I ? 1 : 0;
        t.delChildren += op == OP_D ? 1 : 0;
    }
    [[gnu::noinline]] void push(const FmNode& v) {
        note(v);
        if (sp < stack.size()) stack[sp++] = v;
        else fail("push past fmStackCap (the kernel would set kFlagStack)", ca, split);
    }
};

// what the kernel does with one (pattern, search) item
template <int SIGMA, bool EDIT>
void fmSearch(const Case& c, long ca, uint32_t split, uint32_t pid, uint32_t s, Multiset<Cursor>& leaves,
              std::vector<FmNode>& tasks, Tally& t) {
    Dfs dfs(fmStackCap(c.k, c.sigma), t, ca, split, leaves, tasks);
    const OccLine junk = {{~0u, ~0u, ~0u, ~0u, ~0u}, 0, {~0ull, ~0ull, ~0ull}, 0, 0};  // line B when it is not needed
    FmNode cur = {0, 0, c.n, kDeltaZero};
    bool have = true;
    for (uint64_t guard = 0;; ++guard) {
        if (guard > 50000000) { fail("runaway DFS", ca, split); return; }
        if (!have) {
            if (!dfs.pop(cur)) return;
            have = true;
        }
        if (fmIsLeaf(cur, c.m)) {
            dfs.leaf(pid, cur);
            have = false;
            continue;
        }
        if (split && fmConverts(cur, split)) {
            dfs.convert(pid, s, cur);
            have = false;
            continue;
        }
        const uint32_t se = c.packed[(size_t)s * c.m + cur.pos()];
        const FmDecode d = fmDecode<EDIT>(cur, se, c.pats[(size_t)pid * c.m + schemeQ(se)], true);
        ++t.nodes;
        if (d.needA) {
            ++t.rankNodes;
            t.lines += d.needB ? 2 : 1;
            ++t.needB[d.needB ? 1 : 0];
        }
        // the fetch: the step must not read a line it did not ask for
        const std::vector<OccLine>& occ = d.right ? c.occR : c.occF;
        const OccLine& A = d.needA ? occ[d.lo >> 6] : junk;
        const OccLine& B = d.needB ? occ[d.hi >> 6] : junk;
        dfs.firstPos = d.pos == 0;
        dfs.right = d.right;
        FmNode next;
        have = fmExpand<SIGMA>(cur, d, A.cnt, A.plane, B.cnt, B.plane, c.C.data(), [&](const FmNode& v) { dfs.push(v); }, next);
        if (have) dfs.note(next);
        cur = next;
    }
}

// a text task, as the text kernel starts and runs it, with the whole text as its window
template <bool EDIT>
void textSearch(const Case& c, long ca, uint32_t split, const FmNode& rec, const Packed& T,
                const std::vector<Packed>& P, Multiset<Hit>& hits) {
    const TextTask t = taskOf(rec);
    if (t.hasPos || t.tlen == 0 || t.x >= c.n) { fail("task record does not decode to an SA row", ca, split); return; }
    const uint32_t x = c.sa[t.x];
    const uint32_t cap = 2 * c.k + 2;
    std::vector<TextNode> stack(cap);
    auto row = [&](uint32_t p) -> TextRow {
        const size_t i = (size_t)t.search * c.m + (p < c.m ? p : c.m - 1);
        return {c.table[2 * i], c.table[2 * i + 1]};
    };
    auto pat = [&](uint32_t o, bool fwd) { return P[t.pid].chain(o, fwd, [](long q) { return (uint32_t)(((q * 7 + 3) % 6 + 6) % 6); }); };
    auto win = [&](uint32_t o, bool fwd) { return T.chain(o, fwd, [](long q) { return 1u + (uint32_t)(((q * 5 + 2) % 5 + 5) % 5); }); };
    auto put = [&](uint32_t d, const TextNode& n) {
        if (d >= cap) fail("text stack write past its cap", ca, split);
        else stack[d] = n;
    };
    TextNode cur = textNode(x, x + t.tlen, t.meta);
    uint32_t sp = 0;
    bool have = true;
    for (uint64_t guard = 0;; ++guard) {
        if (guard > 10000000) { fail("runaway text DFS", ca, split); return; }
        if (!have) {
            if (sp == 0) return;
            cur = stack[--sp];
            have = true;
        }
        const TextStepResult r = textStep<EDIT>(cur, sp, true, cap, c.m, c.n, row, pat, win, put);
        if (r.bad || r.sp > cap) { fail("text step: bad set or sp above its cap", ca, split); return; }
        if (r.leaf) ++hits[{t.pid, r.leafStart, r.leafE}];
        cur = r.cur;
        sp = r.sp;
        have = r.have;
    }
}

using FmSearch = void (*)(const Case&, long, uint32_t, uint32_t, uint32_t, Multiset<Cursor>&, std::vector<FmNode>&, Tally&);
using TextSearch = void (*)(const Case&, long, uint32_t, const FmNode&, const Packed&, const std::vector<Packed>&,
                            Multiset<Hit>&);

void runCase(const Case& c, long ca, FmSearch fm, TextSearch text, const Multiset<Cursor>& wantCursors,
             const Multiset<Hit>& wantHits, const uint64_t wantCount[3], Tally& total) {
    const Packed T(c.text);
    std::vector<Packed> P;
    for (uint32_t p = 0; p < c.npat; ++p)
        P.emplace_back(std::vector<uint32_t>(c.pats.begin() + (size_t)p * c.m, c.pats.begin() + (size_t)(p + 1) * c.m));
    for (uint32_t split : {0u, 1u, 4u}) {
        Multiset<Cursor> leaves;
        std::vector<FmNode> tasks;
        Tally t;
        for (uint32_t pid = 0; pid < c.npat; ++pid)
            for (uint32_t s = 0; s < c.ns; ++s) fm(c, ca, split, pid, s, leaves, tasks, t);
        Multiset<Hit> hits;
        for (const auto& lf : leaves)
            for (uint64_t r = lf.first[1]; r < lf.first[1] + lf.first[2]; ++r) hits[{lf.first[0], c.sa[r], lf.first[3]}] += lf.second;
        if (split == 0) {
            if (leaves != wantCursors) fail("leaf cursors differ from the oracle's", ca, split);
            if (t.nodes != wantCount[0]) fail("nodes differ from the oracle's", ca, split);
            if (t.rankNodes != wantCount[1]) fail("rank nodes differ from the oracle's", ca, split);
            if (t.lines != wantCount[2]) fail("extension lines differ from the oracle's", ca, split);
            if (!tasks.empty()) fail("tasks without a split", ca, split);
            total.nodes += t.nodes;
            total.needB[0] += t.needB[0];
            total.needB[1] += t.needB[1];
            total.insChildren += t.insChildren;
            total.delChildren += t.delChildren;
        } else {
            for (const FmNode& rec : tasks) text(c, ca, split, rec, T, P, hits);
            total.tasks += t.tasks;
            if (split == 4) total.multiConversions += t.multiConversions;
        }
        if (hits != wantHits) fail("located hits differ from the oracle's", ca, split);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string word;
    long ca = 0;
    std::map<long, long> items;  // (pattern, search) items per group
    Tally total;
    while (in >> word && word == "case") {
        long group;
        Case c;
        in >> group >> c.sigma >> c.edit >> c.k >> c.m >> c.n >> c.ns >> c.npat;
        if (!in || (c.sigma != 5 && c.sigma != 6) || c.n >= 65536) { std::printf("FAIL: bad case header\n"); return 1; }
        c.C = readRow(in, 8);
        c.occF = occLines(readRow(in, c.n));
        c.occR = occLines(readRow(in, c.n));
        c.sa = readRow(in, c.n);
        c.text = readRow(in, c.n);
        c.pi = readRow(in, (size_t)c.ns * c.m);
        c.l = readRow(in, (size_t)c.ns * c.m);
        c.u = readRow(in, (size_t)c.ns * c.m);
        c.pats = readRow(in, (size_t)c.npat * c.m);
        // the scheme as the library packs it: packScheme per position, then textTable
        c.packed.resize((size_t)c.ns * c.m);
        for (uint32_t s = 0; s < c.ns; ++s)
            for (uint32_t p = 0; p < c.m; ++p) {
                const uint32_t* pi = c.pi.data() + (size_t)s * c.m;
                const uint32_t right = p > 0 ? pi[p] > pi[p - 1] : (c.m > 1 ? pi[1] > pi[0] : 1u);
                c.packed[(size_t)s * c.m + p] = packScheme(pi[p], c.l[(size_t)s * c.m + p], c.u[(size_t)s * c.m + p], right);
            }
        textTable(c.pi.data(), c.l.data(), c.u.data(), c.ns, c.m, c.packed, c.table);
        uint64_t wantCount[3];
        size_t ncur, nhit;
        in >> wantCount[0] >> wantCount[1] >> wantCount[2] >> ncur;
        Multiset<Cursor> wantCursors;
        for (size_t i = 0; i < ncur; ++i) {
            Cursor x;
            in >> x[0] >> x[1] >> x[2] >> x[3];
            ++wantCursors[x];
        }
        in >> nhit;
        Multiset<Hit> wantHits;
        for (size_t i = 0; i < nhit; ++i) {
            Hit x;
            in >> x[0] >> x[1] >> x[2];
            ++wantHits[x];
        }
        if (!in) { std::printf("FAIL: case file truncated\n"); return 1; }
        const FmSearch fm = c.sigma == 5 ? (c.edit ? fmSearch<5, true> : fmSearch<5, false>)
                                         : (c.edit ? fmSearch<6, true> : fmSearch<6, false>);
        runCase(c, ca, fm, c.edit ? textSearch<true> : textSearch<false>, wantCursors, wantHits, wantCount, total);
        items[group] += (long)c.npat * c.ns;
        ++ca;
    }
    if (word != "end") { std::printf("FAIL: case file has no end mark\n"); return 1; }
    for (const auto& g : items) std::printf("group %ld: %ld items\n", g.first, g.second);
    std::printf("nodes %llu, one line %llu, two lines %llu, I children %llu, D children %llu, tasks %llu, conversions of >= 2 rows at split 4: %llu\n",
                (unsigned long long)total.nodes, (unsigned long long)total.needB[0], (unsigned long long)total.needB[1],
                (unsigned long long)total.insChildren, (unsigned long long)total.delChildren, (unsigned long long)total.tasks,
                (unsigned long long)total.multiConversions);
    // what the case writer promised of its cases, seen by the step itself
    if (!total.needB[0] || !total.needB[1]) { std::printf("FAIL: needB was not seen both ways\n"); ++failures; }
    if (!total.insChildren || !total.delChildren) { std::printf("FAIL: no insertion or no deletion child\n"); ++failures; }
    if (!total.multiConversions) { std::printf("FAIL: no conversion of 2 or more rows at split 4\n"); ++failures; }
    std::printf("%s (%ld cases, %d failures)\n", failures ? "FAILED" : "ok", ca, failures);
    return failures ? 1 : 0;
}
