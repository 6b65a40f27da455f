"""tests/loci_model.py, the checker of the loci stage, against rows written by
hand and against the --max_hits restatement of test_golden (CPU)."""
import numpy as np

from loci_model import loci, locus_ids
from test_golden import expected, limit_rows


def rows(*r):
    return np.array(r, np.uint64).reshape(-1, 4)


def same(a, b):
    return np.array_equal(np.asarray(a, np.uint64).reshape(-1, 4), np.asarray(b, np.uint64).reshape(-1, 4))


def test_gap_of_exactly_w_chains_and_w_plus_one_does_not():
    r = rows((0, 0, 10, 2), (0, 0, 13, 1), (0, 0, 17, 0))
    assert same(loci(r, 3), [(0, 0, 13, 1), (0, 0, 17, 0)])      # 13 - 10 = W chains; 17 - 13 = W + 1 does not
    assert same(loci(r, 4), [(0, 0, 17, 0)])
    assert same(loci(r, 2), r)


def test_equal_pos_with_different_e_counts_once_with_the_least():
    r = rows((0, 0, 5, 1), (0, 0, 5, 2), (0, 0, 5, 2), (0, 0, 9, 0), (0, 0, 9, 1))
    assert same(loci(r, 0), [(0, 0, 5, 1), (0, 0, 9, 0)])
    assert same(loci(r, 3), [(0, 0, 5, 1), (0, 0, 9, 0)])        # duplicates at 5 do not stretch the gap to 9
    assert same(loci(r, 4), [(0, 0, 9, 0)])


def test_a_tie_in_e_goes_to_the_smaller_pos():
    r = rows((3, 1, 100, 2), (3, 1, 101, 1), (3, 1, 101, 2), (3, 1, 102, 1), (3, 1, 103, 2))
    assert same(loci(r, 1), [(3, 1, 101, 1)])


def test_seq_id_and_qid_changes_start_a_locus_whatever_the_gap():
    r = rows((0, 0, 50, 1), (0, 1, 51, 0), (1, 1, 51, 0), (1, 1, 52, 1), (2, 0, 0, 2))
    assert same(loci(r, 10), [(0, 0, 50, 1), (0, 1, 51, 0), (1, 1, 51, 0), (2, 0, 0, 2)])
    # a smaller position after a change of record or query (no unsigned wrap of the gap)
    r = rows((0, 0, 900, 0), (0, 1, 2, 0), (1, 0, 1, 0))
    assert same(loci(r, 5), r)
    assert locus_ids(r, 5).tolist() == [0, 1, 2]


def test_w_zero_and_empty_input():
    r = rows((0, 0, 1, 2), (0, 0, 1, 2), (0, 0, 2, 1), (0, 0, 3, 0))
    assert same(loci(r, 0), [(0, 0, 1, 2), (0, 0, 2, 1), (0, 0, 3, 0)])
    assert loci(np.zeros((0, 4), np.uint64), 3).shape == (0, 4)
    assert loci([], 0).shape == (0, 4)
    assert locus_ids([], 0).shape == (0,)


def test_a_long_chain_is_one_locus():
    r = rows(*[(7, 0, p, 2 - (p == 40)) for p in range(0, 300, 2)])
    assert same(loci(r, 2), [(7, 0, 40, 1)])
    assert len(loci(r, 1)) == 150


def test_w_zero_equals_unbounded_max_hits_on_golden():
    for name in ("a_lev_k2", "b_lev_k3"):
        r = expected(name)
        assert np.array_equal(loci(r, 0), limit_rows(r, 10**9)), name


def test_max_hits_over_loci_never_returns_two_rows_of_one_locus():
    for name, W in (("a_lev_k2", 2), ("b_lev_k3", 3), ("a_lev_k2", 0)):
        r = expected(name)
        ids = locus_ids(r, W)
        where = {tuple(x): int(i) for x, i in zip(r[:, :3].tolist(), ids)}
        L = loci(r, W)
        assert len(L) == ids.max() + 1 and len(L) < len(r)
        for n in (1, 2, 3):
            lim = limit_rows(L, n)
            got = [where[tuple(x)] for x in lim[:, :3].tolist()]
            assert len(set(got)) == len(got), (name, W, n)
            assert np.unique(lim[:, 0], return_counts=True)[1].max() <= n
