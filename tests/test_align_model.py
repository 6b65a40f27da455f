"""tests/align_model.py is the alignment rule of docs/semantics.md: checked
against an exhaustive enumeration of transcripts on tiny inputs, against the
oracle's P-set (the e of every position), and for the structure the P0 end
rules promise. No GPU."""
import itertools

import numpy as np
import pytest

import align_model as am
import oracle as O
from helpers import mutate_reads, pset, random_records


def transcripts(P, T, g, K, edit):
    """Every valid transcript of cost <= K: (cost, ref_len, ops), ops over '=XID'."""
    m = len(P)
    JM = am.window(T, g, m, K, edit)
    out = []

    def go(i, j, cost, ops):
        if cost > K:
            return
        if i == m:
            out.append((cost, j, ops))
            return
        if j < JM:
            eq = P[i] == T[g + j]
            go(i + 1, j + 1, cost + (0 if eq else 1), ops + ("=" if eq else "X"))
        if edit:
            go(i + 1, j, cost + 1, ops + "I")
            if 0 < i and j < JM:  # (i < m here): a D is never first or last
                go(i, j + 1, cost + 1, ops + "D")

    go(0, 0, 0, "")
    return out


def ops_of(edits, m):
    ops, i = [], 0
    for qpos, kind in edits:
        ops.extend("=" * (qpos - i))
        i = qpos
        ops.append(" XID"[kind])
        if kind != am.KIND_D:
            i += 1
    ops.extend("=" * (m - i))
    return "".join(ops)


def test_exhaustive_minimum_ref_len_and_priority():
    # texts over {1, 2} with '$' inside; every pattern over {1, 2} of m <= 7 at a sample of positions
    rng = np.random.default_rng(5)
    back = {"=": 0, "X": 0, "I": 1, "D": 2}  # the walk's order of preference at each cell
    checked = aligned = 0
    for _ in range(40):
        recs = [rng.integers(1, 3, size=rng.integers(1, 9)).tolist() for _ in range(rng.integers(1, 4))]
        T = am.concat_text(recs)
        for m in range(1, 8):
            for P in itertools.islice(itertools.product([1, 2], repeat=m), int(rng.integers(0, 3)), None, 5):
                g = int(rng.integers(0, len(T)))
                for K in range(3):
                    for edit in (True, False):
                        all_t = transcripts(P, T, g, K, edit)
                        got = am.align(list(P), T, g, K, edit)
                        checked += 1
                        if not all_t:
                            assert got is None
                            continue
                        aligned += 1
                        e = min(t[0] for t in all_t)
                        ends = sorted({(abs(t[1] - m), t[1]) for t in all_t if t[0] == e})
                        ref_len = ends[0][1]
                        best = min((t for t in all_t if t[0] == e and t[1] == ref_len),
                                   key=lambda t: [back[o] for o in reversed(t[2])])
                        assert got is not None and (got[0], got[1]) == (e, ref_len), (P, T, g, K, edit)
                        assert ops_of(got[2], m) == best[2], (P, T, g, K, edit, got, best)
                        assert am.apply(list(P), T, g, got[1], got[2])
    assert checked > 3000 and aligned > 300


CONFIGS = [(sigma, m, k, edit) for sigma in (5, 6) for m, k in ((6, 0), (8, 1), (11, 2), (13, 3), (9, 3), (7, 2))
           for edit in (True, False)]


@pytest.mark.parametrize("sigma,m,k,edit", CONFIGS)
def test_e_star_is_the_p_set(sigma, m, k, edit):
    rng = np.random.default_rng(100 * sigma + 10 * m + k + edit)
    recs = random_records(rng, [260, 90, 120], sigma, with_n=True, repeats=True)
    recs.append(np.resize(np.array([1, 2, 2], np.uint8), 60))  # a period-3 record
    recs.append(np.full(25, 3, np.uint8))                      # a homopolymer
    reads = np.concatenate([mutate_reads(rng, recs[:3], 12, m, k, sigma),
                            np.resize(np.array([2, 2, 1], np.uint8), m)[None, :],
                            np.full((1, m), 3, np.uint8)])
    want = pset(np.asarray(O.bruteforce(recs, reads, k, edit=edit), np.uint64).reshape(-1, 4))
    T = am.concat_text(recs)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])
    got = {}
    for q, P in enumerate(reads.tolist()):
        for s, r in enumerate(recs):
            for pos in range(len(r)):
                res = am.align(P, T, int(starts[s]) + pos, k, edit)
                if res is not None:
                    got[(q, s, pos)] = res[0]
                    assert am.apply(P, T, int(starts[s]) + pos, res[1], res[2])
    assert len(want) > 10
    assert got == want


def test_no_leading_or_trailing_d_and_no_i_next_to_d():
    rng = np.random.default_rng(9)
    n = 0
    for _ in range(60):
        recs = [np.resize(rng.integers(1, 4, size=rng.integers(1, 4)), rng.integers(30, 80)).astype(np.uint8),
                rng.integers(1, 4, size=70).astype(np.uint8)]
        T = am.concat_text(recs)
        for _ in range(40):
            m, K = int(rng.integers(4, 40)), int(rng.integers(0, 5))
            g = int(rng.integers(0, len(T)))
            P = mutate_reads(rng, recs, 1, m, min(K, 3), 5)[0].tolist() if rng.random() < 0.5 else \
                [x if x else 1 for x in (T[g:g + m] + [1] * m)[:m]]
            if rng.random() < 0.7 and m > 6:
                del P[int(rng.integers(m))]
                P.append(int(rng.integers(1, 4)))
            res = am.align(P, T, g, K, True)
            if res is None:
                continue
            n += 1
            ops = ops_of(res[2], m)
            assert ops[0] != "D" and ops[-1] != "D", ops
            assert "ID" not in ops and "DI" not in ops, ops
            assert res[1] == m - ops.count("I") + ops.count("D")
            assert am.apply(P, T, g, res[1], res[2])
    assert n > 400


def test_worked_example_is_left_aligned():
    code = {"A": 1, "C": 2, "G": 3, "T": 5}
    T = am.concat_text([[code[c] for c in "ACGTTTTTGA"]])
    P = [code[c] for c in "ACGTTTTGA"]
    e, ref_len, edits = am.align(P, T, 0, 2, True)
    assert (e, ref_len) == (1, 10)
    assert am.cigar(edits, len(P)) == "3=1D6="
    assert am.record_of((e, ref_len, edits)) == (1, 10, [(3 << 2) | 3, 0, 0, 0, 0, 0, 0, 0])
