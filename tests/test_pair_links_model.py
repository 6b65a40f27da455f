"""tests/pair_links_model.py, the checker of the pair stage's links
(docs/semantics.md "Pair links"), on rows written by hand and on the planted
case's oracle rows for every setting and delta: the rule's promises, the
shapes planted by name, and sahara_pair_mapq's table against the model's
(CPU)."""
import numpy as np
import pytest

import sahara_amd as sa
from best_pairs_case import DELTAS, SETTINGS, planted
from best_pairs_model import NONE
from pair_links_case import check, expected_links
from pair_links_model import LINK_DTYPE, PRIMARY, mapq, pair_links


def rows(*r):
    return np.array(r, np.uint64).reshape(-1, 4)


def test_links_by_hand():
    # pair 1: A at 100 sees rc B at 200 (0) and at 340 (1); A at 280 sees the one at 340 only
    r = rows((4, 0, 100, 0), (4, 0, 280, 0), (7, 0, 200, 0), (7, 0, 340, 1))
    kept, summary, links, info = pair_links(r, 48, 100, 300, 1)
    assert len(kept) == 4 and links.dtype == LINK_DTYPE
    assert links["mate"].tolist() == [2, 2, -2, -3]      # the dear B at 340 sees both A's and takes the first
    assert links["score"].tolist() == [0, 1, 0, 1]
    assert links["flags"].tolist() == [PRIMARY, 0, PRIMARY, 0]
    assert links["mapq"].tolist() == [10, 0, 10, 0]       # one best placement, next = best + 1
    assert info["mutual"].tolist() == [True, False, True, False]  # (A at 280 -> B at 340 -> A at 100)
    assert info["n_best"].tolist() == [0, 1] and info["mapq"].tolist() == [0, 10]
    # delta 0: the best placement alone
    kept, summary, links, info = pair_links(r, 48, 100, 300, 0)
    assert links["mate"].tolist() == [1, -1] and links["flags"].tolist() == [PRIMARY, PRIMARY]
    assert links["mapq"].tolist() == [10, 10]


def test_a_tie_on_one_strand_alone_is_a_tie():
    # one forward record, two reverse ones at the same total: n_best = max(1, 2)
    r = rows((0, 0, 100, 0), (3, 0, 200, 0), (3, 0, 300, 0))
    kept, summary, links, info = pair_links(r, 48, 48, 1000, 0)
    assert info["n_best"].tolist() == [2]
    assert links["mate"].tolist() == [1, -1, -2] and links["flags"].tolist() == [PRIMARY, PRIMARY, 0]
    assert links["mapq"].tolist() == [1, 1, 0]
    # duplicates of a position: the link goes to the first, which is the kept one
    r = rows((0, 0, 100, 0), (0, 0, 100, 2), (3, 0, 200, 1), (3, 0, 200, 2))
    kept, summary, links, info = pair_links(r, 48, 48, 1000, 30)
    assert links["mate"].tolist() == [1, -1] and links["mapq"].tolist() == [60, 60]
    # nothing kept: no links
    assert len(pair_links(r, 48, 48, 100, 0, n_pairs=2)[2]) == 0


def test_the_library_mapq_is_the_models_table():
    for best in list(range(0, 32)) + [NONE]:
        for nxt in list(range(best + 1, best + 9)) + [NONE]:
            if best != NONE and nxt <= best:
                continue
            for n in (0, 1, 2, 3, 4, 64, 65535):
                assert sa.pair_mapq(best, min(nxt, NONE), n) == mapq(best, min(nxt, NONE), n), (best, nxt, n)
    assert mapq(0, 1, 1) == 10 and mapq(4, NONE, 1) == 60 and mapq(0, 9, 1) == 60 and mapq(0, 1, 2) == 1
    assert mapq(0, NONE, 3) == 0 and mapq(NONE, NONE, 0) == 0


def test_the_planted_case_holds_what_the_gpu_tests_rely_on():
    check()


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("setting", SETTINGS)
def test_promises_on_the_planted_rows(setting, delta):
    c = planted()
    kept, summary, links, info = expected_links(setting, delta)  # (the model asserts: every mate is kept)
    assert len(links) == len(kept) and (links["reserved"] == 0).all()
    at = np.arange(len(kept))
    there = at + links["mate"]
    pair = (kept[:, 0] >> np.uint64(2)).astype(np.int64)
    # the mate's offset stays within its pair's records, and on the other strand
    assert ((there >= 0) & (there < len(kept))).all() and (pair[there] == pair).all()
    assert ((kept[there, 0] ^ kept[:, 0]) == 3).all() and (kept[there, 1] == kept[:, 1]).all()
    assert (links["score"] == kept[:, 3] + kept[there, 3]).all()
    # one primary even-qid and one primary odd-qid record per pair with kept hits
    prim = (links["flags"] & PRIMARY) != 0
    odd = (kept[:, 0] & np.uint64(1)).astype(bool)
    with_hits = np.unique(pair)
    assert np.array_equal(np.bincount(pair[prim & ~odd], minlength=c["n_pairs"])[with_hits], np.ones(len(with_hits)))
    assert np.array_equal(np.bincount(pair[prim & odd], minlength=c["n_pairs"])[with_hits], np.ones(len(with_hits)))
    assert np.array_equal(with_hits, np.flatnonzero(summary["best"] != NONE))
    # the primary's score is best, its link is mutual, and the two point at each other
    assert (links["score"][prim] == summary["best"][pair[prim]]).all()
    assert info["mutual"][prim].all() and prim[there[prim]].all()
    # secondary records carry no MAPQ; primaries the pair's, which does not depend on delta
    assert (links["mapq"][~prim] == 0).all()
    assert (links["mapq"][prim] == info["mapq"][pair[prim]]).all()
    assert np.array_equal(info["mapq"], expected_links(setting, 0)[3]["mapq"])
    assert np.array_equal(info["n_best"], expected_links(setting, 0)[3]["n_best"])
    assert set(np.unique(info["mapq"]).tolist()) <= {0, 1, 10, 20, 30, 40, 50, 60}
