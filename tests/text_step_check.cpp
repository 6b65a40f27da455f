// The text kernel's micro-step (csrc/text_step.h: textStep) run on the host as
// a DFS — pop, step, stack — over the cases that tests/test_text_step.py
// writes: per task the leaves must equal the plain P0 DFS's and the nodes
// processed the model's (tests/text_model.py chain()), the stack must stay
// within stackCap and `bad` unset. The readers return junk outside the pattern
// and outside the window, as the kernel's LDS does. Built under the address
// and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../sahara_amd/csrc/text_step.h"
#include "planes_host.h"

using namespace sahara;

namespace {

int failures = 0;
void fail(const char* what, long ca, long task) {
    if (++failures <= 20) std::printf("FAIL case %ld task %ld: %s\n", ca, task, what);
}

int pymod(long v, long n) { return (int)(((v % n) + n) % n); }

std::vector<uint32_t> readRow(std::istream& in, size_t n) {
    std::vector<uint32_t> v(n);
    for (auto& x : v) in >> x;
    return v;
}

template <bool EDIT>
void runTask(long ca, long task, const TextNode& start, uint32_t cap, uint32_t m, const std::vector<uint32_t>& table,
             const Packed& P, const Packed& T, std::map<std::pair<uint32_t, uint32_t>, long>& leaves, long& steps) {
    std::vector<TextNode> stack(cap);
    auto row = [&](uint32_t p) -> TextRow {
        if (p >= m) { fail("table row past the scheme", ca, task); p = m - 1; }
        return {table[2 * (size_t)p], table[2 * (size_t)p + 1]};
    };
    // beyond the pattern: the rule of text_model.py; outside the window:
    // symbols (non-zero), which only the step's `avail` mask keeps out
    auto pat = [&](uint32_t o, bool fwd) { return P.chain(o, fwd, [](long q) { return (uint32_t)pymod(q * 7 + 3, 6); }); };
    auto win = [&](uint32_t o, bool fwd) { return T.chain(o, fwd, [](long q) { return 1u + (uint32_t)pymod(q * 5 + 2, 5); }); };
    auto put = [&](uint32_t d, const TextNode& n) {
        if (d >= cap) fail("stack write past stackCap", ca, task);
        else stack[d] = n;
    };
    TextNode cur = start;
    uint32_t sp = 0;
    bool have = true;
    for (;;) {
        if (!have) {
            if (sp == 0) break;
            cur = stack[--sp];
            have = true;
        }
        const TextStepResult r = textStep<EDIT>(cur, sp, true, cap, m, (uint32_t)T.n, row, pat, win, put);
        ++steps;
        if (r.bad) fail("bad set", ca, task);
        if (r.sp > cap) fail("sp above stackCap", ca, task);
        if (r.leaf) ++leaves[{r.leafStart, r.leafE}];
        if (r.steps + (r.leaf ? 1u : 0u) != 1u) fail("a live step is a node or a leaf", ca, task);
        cur = r.cur;
        sp = r.sp > cap ? cap : r.sp;
        have = r.have;
        if (steps > 10000000) { fail("runaway DFS", ca, task); break; }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::map<long, long> perGroup, needOf;  // tasks checked per group, and the number it must exceed
    std::string word;
    long ca = 0;
    while (in >> word && word == "case") {
        long group, need, ntasks;
        uint32_t m, nT, edit, cap;
        in >> group >> need >> m >> nT >> edit >> cap >> ntasks;
        needOf[group] = need;
        const std::vector<uint32_t> pi = readRow(in, m), l = readRow(in, m), u = readRow(in, m);
        const Packed P(readRow(in, m)), T(readRow(in, nT));
        // the rows as the library builds them: packScheme per position, then textTable
        std::vector<uint32_t> packed(m), table;
        for (uint32_t p = 0; p < m; ++p) {
            const uint32_t right = p > 0 ? pi[p] > pi[p - 1] : (m > 1 ? pi[1] > pi[0] : 1u);
            packed[p] = packScheme(pi[p], l[p], u[p], right);
        }
        textTable(pi.data(), l.data(), u.data(), 1, m, packed, table);
        for (long t = 0; t < ntasks; ++t) {
            uint32_t xs, ye, pos, e, lL, lR;
            long wantSteps, nleaf;
            in >> xs >> ye >> pos >> e >> lL >> lR >> wantSteps >> nleaf;
            std::map<std::pair<uint32_t, uint32_t>, long> want, got;
            for (long i = 0; i < nleaf; ++i) {
                uint32_t lx, le;
                long n;
                in >> lx >> le >> n;
                want[{lx, le}] = n;
            }
            if (!in) { std::printf("FAIL: case file truncated\n"); return 1; }
            const TextNode start = textNode(xs, ye, pos | (e << 16) | (lL << 20) | (lR << 22));
            long steps = 0;
            if (edit) runTask<true>(ca, t, start, cap, m, table, P, T, got, steps);
            else runTask<false>(ca, t, start, cap, m, table, P, T, got, steps);
            if (got != want) fail("leaf multiset differs from plain()", ca, t);
            if (steps != wantSteps) fail("nodes processed differ from the model's steps", ca, t);
            ++perGroup[group];
        }
        ++ca;
    }
    if (word != "end") { std::printf("FAIL: case file has no end mark\n"); return 1; }
    for (const auto& g : perGroup) {
        std::printf("group %ld: %ld tasks\n", g.first, g.second);
        if (g.second <= needOf[g.first]) {
            std::printf("FAIL: group %ld checked %ld tasks (<= %ld)\n", g.first, g.second, needOf[g.first]);
            ++failures;
        }
    }
    if (perGroup.size() != 6) { std::printf("FAIL: %zu groups, not 6\n", perGroup.size()); ++failures; }
    std::printf("%s (%ld cases, %d failures)\n", failures ? "FAILED" : "ok", ca, failures);
    return failures ? 1 : 0;
}
