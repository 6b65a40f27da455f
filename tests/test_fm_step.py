"""The FM kernel's node step itself (csrc/fm_step.h, the code a lane runs) on a
CPU: tests/fm_step_check.cpp runs it as a DFS from the root over small indexes
stated by tests/index_model.py and holds it to the oracle — leaf cursors,
located hits and the node / rank-node / Occ-line counts without a split, and
with split 1 and 4 the union of FM leaves and of the text tasks' leaves
(csrc/text_step.h finishes each task) to the located hits. Built alone under
the address and undefined-behaviour sanitizers."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle as O  # noqa: E402
from index_model import model  # noqa: E402

OP_NONE, OP_MS, OP_I, OP_D = 0, 1, 2, 3

# (group, sigma, edit, k, generator, m, record lengths, patterns, seed): the
# smallest that can still go wrong: texts of 150-600 symbols in 1-5 records,
# made of repeats so that intervals exceed the splits and cross 64-row lines
GROUPS = [
    (1, 5, False, 0, "backtracking", 8, [150], 120, 11),
    (2, 5, False, 1, "pigeon", 12, [200, 90, 60], 60, 12),
    (3, 6, False, 2, "h2-k2", 16, [260, 180, 1, 100, 59], 40, 13),
    (4, 5, True, 1, "pigeon", 12, [170, 130], 60, 14),
    (5, 6, True, 2, "h2-k2", 20, [300, 150, 150], 40, 15),
    (6, 6, True, 3, "pigeon", 24, [150, 80], 30, 16),
    (7, 5, False, 3, "backtracking", 10, [400], 110, 17),
]


def make_records(rng, sigma, lens):
    """Records cut from mutated copies of a few short units (repeats); at sigma 6 with N (4) among them."""
    syms = [c for c in range(1, sigma) if not (sigma == 6 and c == 4)]
    units = [rng.choice(syms, size=int(rng.integers(7, 30))) for _ in range(3)]
    recs = []
    for n in lens:
        out = []
        while len(out) < n:
            u = units[int(rng.integers(len(units)))].copy()
            for _ in range(int(rng.integers(0, 3))):
                u[int(rng.integers(len(u)))] = rng.choice(syms)
            out += list(u)
        r = np.array(out[:n], np.uint8)
        if sigma == 6 and n > 20:
            r[int(rng.integers(n))] = 4
        recs.append(r)
    return recs


def make_patterns(rng, recs, sigma, m, k, edit, npat):
    """Windows of the records with up to k substitutions (edit: or insertions / deletions); a few with an N."""
    pats = []
    long_recs = [r for r in recs if len(r) > m + k + 1]
    for i in range(npat):
        r = long_recs[int(rng.integers(len(long_recs)))]
        s = int(rng.integers(len(r) - m - k))
        w = list(r[s:s + m + k])
        for _ in range(i % (k + 1)):
            op = int(rng.integers(3)) if edit else 0
            at = int(rng.integers(1, m - 1))
            if op == 0:
                w[at] = int(rng.integers(1, sigma))
            elif op == 1:
                w.insert(at, int(rng.integers(1, sigma)))
            else:
                del w[at]
        if sigma == 6 and i % 9 == 4:
            w[int(rng.integers(m))] = 4
        pats.append(w[:m])
    return np.array(pats, np.uint8)


def child_kinds(M, sigma, P, pi, l, u, edit):
    """Searcher::visit (oracle/oracle.cpp) restated over the model's BWTs, only as far as it takes to see
    which kinds of children the DFS of this (pattern, search) creates: the set of OP_* of its children."""
    n, m = M["n"], len(pi)
    cum = {side: [np.concatenate([[0], np.cumsum(M[side] == c)]) for c in range(sigma)] for side in ("bwt_f", "bwt_r")}
    right_at = [pi[p] > pi[p - 1] for p in range(1, m)]
    right_at = [right_at[0] if m > 1 else True] + right_at
    seen = set()
    stack = [(0, 0, n, 0, 0, OP_NONE, OP_NONE)]
    while stack and not {OP_I, OP_D} <= seen:
        lb, lbr, ln, pos, e, lastL, lastR = stack.pop()
        if pos == m:
            continue
        right = right_at[pos]
        side = lastR if right else lastL
        match_ok = l[pos] <= e <= u[pos]
        mis_ok = l[pos] <= e + 1 <= u[pos]
        del_ok = edit and pos > 0 and e + 1 <= u[pos] and side != OP_I
        ins_ok = edit and mis_ok and side != OP_D
        sides = lambda op: (op, op) if pos == 0 else ((lastL, op) if right else (op, lastR))  # noqa: E731
        if match_ok or mis_ok or del_ok:
            tab = cum["bwt_r" if right else "bwt_f"]
            lo = lbr if right else lb
            occ = [0] + [int(tab[c][lo + ln] - tab[c][lo]) for c in range(1, sigma)]
            acc = (lb if right else lbr) + (ln - sum(occ))
            for c in range(1, sigma):
                base = int(M["C"][c]) + int(tab[c][lo])
                ch = (acc, base, occ[c]) if right else (base, acc, occ[c])
                acc += occ[c]
                if not occ[c]:
                    continue
                if c == P[pi[pos]]:
                    if match_ok:
                        stack.append(ch + (pos + 1, e) + sides(OP_MS))
                elif mis_ok:
                    stack.append(ch + (pos + 1, e + 1) + sides(OP_MS))
                if del_ok:
                    seen.add(OP_D)
                    stack.append(ch + (pos, e + 1) + sides(OP_D))
        if ins_ok:
            seen.add(OP_I)
            stack.append((lb, lbr, ln, pos + 1, e + 1) + sides(OP_I))
    return seen


def write_cases(path):
    lines = []
    multi = 0   # leaf cursors of 2-4 rows: the first node of at most 4 rows on such a leaf's path has at
                # least as many (an interval never grows down a path), so split = 4 converts it into >= 2 tasks
    left_first = False
    for group, sigma, edit, k, gen, m, lens, npat, seed in GROUPS:
        rng = np.random.default_rng(seed)
        recs = make_records(rng, sigma, lens)
        pats = make_patterns(rng, recs, sigma, m, k, edit, npat)
        M = model(recs, sigma, 16)
        assert 150 <= M["n"] <= 600 + len(lens) and 1 <= len(lens) <= 5 and 8 <= m <= 24
        sch = O.scheme(gen, 0, k, m, hamming=not edit)
        pi, l, u = sch
        idx = O.Index.build(recs, sigma, 16)
        hits, cnt = idx.search(pats, sch, edit=edit, locate=True)
        cursors, _ = idx.search(pats, sch, edit=edit, locate=False)
        # ---- a thin case set fails here, loudly
        assert npat * len(pi) > 100, (group, npat * len(pi))
        assert set(int(e) for e in hits[:, 3]) == set(range(k + 1)), (group, sorted(set(hits[:, 3])))
        # some ranked node reads one line (ext_lines < 2 rank_nodes) and some two (ext_lines > rank_nodes)
        assert cnt["rank_nodes"] < cnt["ext_lines"] < 2 * cnt["rank_nodes"], (group, cnt)
        if edit:
            kinds = set()
            for p in range(min(npat, 8)):
                for s in range(len(pi)):
                    kinds |= child_kinds(M, sigma, pats[p], pi[s], l[s], u[s], True)
            assert {OP_I, OP_D} <= kinds, (group, kinds)
        multi += int(np.sum((cursors[:, 2] >= 2) & (cursors[:, 2] <= 4)))
        left_first = left_first or any(int(pi[s][1]) < int(pi[s][0]) for s in range(len(pi)))
        starts = np.concatenate([[0], np.cumsum(M["rec_lens"] + 1)]).astype(np.uint64)
        lines.append("case %d %d %d %d %d %d %d %d" % (group, sigma, int(edit), k, m, M["n"], len(pi), npat))
        rows = [list(M["C"]) + [0] * (8 - len(M["C"])), M["bwt_f"], M["bwt_r"], M["sa"], M["text"],
                pi.ravel(), l.ravel(), u.ravel(), pats.ravel(),
                [cnt["nodes"], cnt["rank_nodes"], cnt["ext_lines"], len(cursors)], cursors.ravel(), [len(hits)],
                np.stack([hits[:, 0], starts[hits[:, 1].astype(np.int64)] + hits[:, 2], hits[:, 3]], 1).ravel()]
        for row in rows:
            lines.append(" ".join(str(int(v)) for v in row))
    assert multi > 0 and left_first, (multi, left_first)
    lines.append("end")
    path.write_text("\n".join(lines) + "\n")


def test_fm_step_on_host(tmp_path):
    exe = tmp_path / "fm_step_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "fm_step_check.cpp"), "-o", str(exe)], check=True)
    cases = tmp_path / "cases.txt"
    write_cases(cases)
    p = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
