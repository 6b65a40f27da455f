"""tests/best_pairs_model.py, the checker of the pair stage's best mode,
against rows written by hand and against a direct restatement of
docs/semantics.md "Best pairs" (every hit of a pair against every other,
O(n^2) per pair) on the planted case's oracle rows; the rule's identities; and
the planted case's own assertions (CPU)."""
import numpy as np
import pytest

from best_pairs_case import DELTAS, M, SETTINGS, WIDE, check, expected, planted
from best_pairs_model import NONE, SUMMARY_DTYPE, best_pairs, stats_of
from pairs_model import pairs


def rows(*r):
    return np.array(r, np.uint64).reshape(-1, 4)


def same(a, b):
    return np.array_equal(np.asarray(a, np.uint64).reshape(-1, 4), np.asarray(b, np.uint64).reshape(-1, 4))


def restated(r, length, min_fragment, max_fragment, delta, n_pairs):
    """Scores all against all within a pair, in blocks of rows; then the rule
    pair by pair in plain Python."""
    r = np.asarray(r, np.uint64).reshape(-1, 4)
    least = max(min_fragment, length)
    q, s, p, e = (r[:, i].astype(np.int64) for i in range(4))
    m = np.full(len(r), NONE, np.int64)
    pair = q >> 2
    edges = np.flatnonzero(np.diff(pair, prepend=-1, append=-1))
    keep = np.zeros(len(r), bool)
    summary = np.zeros(n_pairs, SUMMARY_DTYPE)
    summary["best"] = summary["next"] = NONE
    for a, b in zip(edges[:-1].tolist(), edges[1:].tolist()):
        i = np.arange(a, b)
        for lo in range(0, len(i), 512):
            x = i[lo:lo + 512][:, None]
            y = i[None, :]
            fwd = np.where(q[x] % 2 == 0, p[x], p[y])
            rev = np.where(q[x] % 2 == 0, p[y], p[x])
            frag = rev + length - fwd
            ok = ((q[x] ^ 3) == q[y]) & (s[x] == s[y]) & (rev >= fwd) & (frag >= least) & (frag <= max_fragment)
            cost = np.where(ok, e[y], NONE).min(axis=1)
            m[i[lo:lo + 512]] = np.where(cost == NONE, NONE, e[i[lo:lo + 512]] + cost)
        seen, valued = set(), []
        for j in range(a, b):
            key = (q[j], s[j], p[j])
            if key not in seen and m[j] != NONE:
                valued.append(j)
            seen.add(key)
        if not valued:
            continue
        s1 = min(m[j] for j in valued)
        above = [m[j] for j in valued if m[j] > s1]
        kept = [j for j in valued if m[j] <= s1 + delta]
        keep[kept] = True
        summary[pair[a]] = (s1, min(above) if above else NONE, min(65535, sum(q[j] % 2 == 0 for j in kept)),
                            min(65535, sum(q[j] % 2 == 1 for j in kept)), 0)
    return r[keep], summary


def test_scores_and_slack_by_hand():
    # pair 0: A at 100 (qid 0), rc B at 200 (0 errors) and at 300 (2 errors); len 48
    r = rows((0, 0, 100, 1), (3, 0, 200, 0), (3, 0, 300, 2))
    for delta, want in ((0, r[:2]), (1, r[:2]), (2, r)):
        k, s = best_pairs(r, 48, 48, 1000, delta)
        assert same(k, want)
        assert tuple(s[0]) == (1, 3, 1, len(want) - 1, 0)
    # nothing concordant: nothing kept, and the summary says so; a pair without rows is there too
    k, s = best_pairs(r, 48, 48, 100, 0, n_pairs=3)
    assert same(k, []) and [tuple(x) for x in s] == [(NONE, NONE, 0, 0, 0)] * 3


def test_duplicates_of_a_position_keep_the_first_and_cost_the_least():
    r = rows((0, 0, 100, 0), (0, 0, 100, 2), (3, 0, 200, 1), (3, 0, 200, 2))
    k, s = best_pairs(r, 48, 48, 1000, 30)
    assert same(k, [r[0], r[2]]) and tuple(s[0]) == (1, NONE, 1, 1, 0)


def test_both_orientations_compete_in_one_minimum():
    # A with rc B at a cost of 0 + 1, B with rc A at 2 + 0
    r = rows((0, 0, 100, 0), (1, 0, 900, 0), (2, 0, 800, 2), (3, 0, 200, 1))
    k, s = best_pairs(r, 48, 48, 1000, 0)
    assert same(k, [r[0], r[3]]) and tuple(s[0]) == (1, 2, 1, 1, 0)
    k, s = best_pairs(r, 48, 48, 1000, 1)
    assert same(k, r) and tuple(s[0]) == (1, 2, 2, 2, 0)


def test_a_dear_mate_shared_by_two_forward_hits():
    # A at 100 sees rc B at 200 (0) and at 340 (1); A at 280 sees the one at 340 only
    r = rows((4, 0, 100, 0), (4, 0, 280, 0), (7, 0, 200, 0), (7, 0, 340, 1))
    k, s = best_pairs(r, 48, 100, 300, 0)
    assert same(k, [r[0], r[2]]) and tuple(s[1]) == (0, 1, 1, 1, 0) and tuple(s[0]) == (NONE, NONE, 0, 0, 0)
    assert same(best_pairs(r, 48, 100, 300, 1)[0], r)


def test_bad_arguments():
    with pytest.raises(ValueError):
        best_pairs(rows(), 48, 0, 100, 31)
    with pytest.raises(ValueError):
        best_pairs(rows(), 48, 0, 47, 0)
    k, s = best_pairs(rows(), 48, 0, 100, 0)
    assert k.shape == (0, 4) and len(s) == 0 and stats_of(k, s) == (0, 0, 0)


def test_the_planted_case_holds_what_the_gpu_tests_rely_on():
    check()


@pytest.mark.parametrize("setting", SETTINGS)
def test_identities_on_the_planted_rows(setting):
    w = planted()["want"]
    paired = pairs(w, M, *setting)
    in_pairs = set(map(tuple, paired.tolist()))
    for delta in DELTAS:
        kept, summary = expected(setting, delta)
        assert set(map(tuple, kept.tolist())) <= in_pairs
        # every kept row has a kept mate: the pair rule keeps all of the kept rows
        assert np.array_equal(pairs(kept, M, *setting), kept)
        n_kept, n_pairs, _ = stats_of(kept, summary)
        assert n_kept == int(summary["n_fwd"].sum()) + int(summary["n_rev"].sum())
        assert n_pairs == len(np.unique(kept[:, 0] >> np.uint64(2)))
    # delta = 30: the pair rule's rows, each position once with its least err
    head = np.ones(len(paired), bool)
    head[1:] = (paired[1:, :3] != paired[:-1, :3]).any(axis=1)
    assert np.array_equal(expected(setting, 30)[0], paired[head])


@pytest.mark.parametrize("delta", DELTAS)
def test_model_equals_the_rule_restated_on_the_planted_rows(delta):
    c = planted()
    kept, summary = restated(c["want"], M, *WIDE, delta, c["n_pairs"])
    assert np.array_equal(expected(WIDE, delta)[0], kept)
    assert np.array_equal(expected(WIDE, delta)[1], summary)
