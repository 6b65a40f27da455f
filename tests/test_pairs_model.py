"""tests/pairs_model.py, the checker of the pair stage, against rows written by
hand and against a direct restatement of docs/semantics.md "Pairs" (every hit
of a pair against every other, O(n^2) per pair) on the planted case's oracle
rows; and the planted case's own assertions (CPU)."""
import numpy as np
import pytest

from pairs_case import M, SETTINGS, check, kept, planted
from pairs_model import pair_count, pairs


def rows(*r):
    return np.array(r, np.uint64).reshape(-1, 4)


def same(a, b):
    return np.array_equal(np.asarray(a, np.uint64).reshape(-1, 4), np.asarray(b, np.uint64).reshape(-1, 4))


def restated(r, length, min_fragment, max_fragment):
    """A hit is kept iff some hit of the call is concordant with it: all
    against all within a pair, in blocks of rows."""
    r = np.asarray(r, np.uint64).reshape(-1, 4)
    least = max(min_fragment, length)
    q, s, p = (r[:, i].astype(np.int64) for i in range(3))
    keep = np.zeros(len(r), bool)
    pair = q >> 2
    edges = np.flatnonzero(np.diff(pair, prepend=-1, append=-1))
    for a, b in zip(edges[:-1].tolist(), edges[1:].tolist()):
        i = np.arange(a, b)
        for lo in range(0, len(i), 512):
            x = i[lo:lo + 512][:, None]
            y = i[None, :]
            # x against y: partners, one record; the even one is the forward mate
            fwd = np.where(q[x] % 2 == 0, p[x], p[y])
            rev = np.where(q[x] % 2 == 0, p[y], p[x])
            frag = rev + length - fwd
            ok = ((q[x] ^ 3) == q[y]) & (s[x] == s[y]) & (rev >= fwd) & (frag >= least) & (frag <= max_fragment)
            keep[i[lo:lo + 512]] = ok.any(axis=1)
    return r[keep]


def test_window_edges_by_hand():
    # pair 0: A at 100 (qid 0), rc B at 152 / 352 / 353 (qid 3); len 48: fragments 100, 300, 301
    r = rows((0, 0, 100, 0), (3, 0, 152, 0), (3, 0, 352, 1), (3, 0, 353, 2))
    assert same(pairs(r, 48, 100, 300), r[:3])
    assert same(pairs(r, 48, 101, 300), [r[0], r[2]])
    assert same(pairs(r, 48, 101, 299), [])
    assert same(pairs(r, 48, 301, 301), [r[0], r[3]])
    assert same(pairs(r, 48, 0, 48), [])


def test_fragment_equal_to_len_and_min_below_len():
    r = rows((4, 1, 7, 0), (7, 1, 7, 2), (7, 1, 8, 2))
    assert same(pairs(r, 48, 48, 48), r[:2])
    assert same(pairs(r, 48, 0, 48), r[:2])      # min_fragment below len counts as len
    assert same(pairs(r, 48, 0, 49), r)
    assert same(pairs(r, 48, 49, 49), [r[0], r[2]])


def test_orientation_record_and_partner():
    # rc mate left of the forward mate; another record; both forward (qids 0 and 2); rc A with B (1 and 2)
    assert same(pairs(rows((0, 0, 500, 0), (3, 0, 300, 0)), 48, 0, 1000), [])
    assert same(pairs(rows((0, 0, 100, 0), (3, 1, 200, 0)), 48, 0, 1000), [])
    assert same(pairs(rows((0, 0, 100, 0), (2, 0, 200, 0)), 48, 0, 1000), [])
    r = rows((1, 0, 200, 1), (2, 0, 100, 0))
    assert same(pairs(r, 48, 0, 1000), r)
    assert same(pairs(rows((1, 0, 100, 1), (2, 0, 200, 0)), 48, 0, 1000), [])
    # partners of different pairs never meet
    assert same(pairs(rows((0, 0, 100, 0), (7, 0, 200, 0)), 48, 0, 1000), [])


def test_duplicates_stay_together_and_positions_near_zero():
    r = rows((1, 0, 10, 0), (1, 0, 10, 2), (1, 0, 60, 1), (2, 0, 8, 0), (2, 0, 8, 1))
    # dmin = 52: rc A at 10 has no room to its left; at 60 the forward mate at 8 is exactly dmin away
    assert same(pairs(r, 48, 100, 300), r[2:])
    assert same(pairs(r, 48, 48, 60), [r[0], r[1], r[3], r[4]])
    assert pair_count(r) == 1 and pair_count(rows((0, 0, 1, 0), (5, 0, 1, 0), (7, 0, 1, 0))) == 2
    assert pairs([], 48, 0, 100).shape == (0, 4)
    with pytest.raises(ValueError):
        pairs(r, 48, 0, 47)
    with pytest.raises(ValueError):
        pairs(r, 48, 200, 100)


def test_the_planted_case_holds_what_the_gpu_tests_rely_on():
    check()


@pytest.mark.parametrize("setting", SETTINGS)
def test_model_equals_the_rule_restated_on_the_planted_rows(setting):
    w = planted()["want"]
    assert np.array_equal(kept(setting), restated(w, M, *setting))
