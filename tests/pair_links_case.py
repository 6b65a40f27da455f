"""The planted case of the pair-links tests: tests/best_pairs_case.py's, with
the model's links (tests/pair_links_model.py) on the oracle's rows, computed
once per setting and delta. check() asserts what the GPU tests rely on: each
shape that the rule (docs/semantics.md "Pair links") distinguishes is in the
case by name. No GPU: tests/test_pair_links_gpu.py runs it on one."""
import functools

import numpy as np

import best_pairs_case as bp
from best_pairs_case import DELTAS, M, SETTINGS, WIDE
from pair_links_model import PRIMARY, pair_links


@functools.lru_cache(maxsize=None)
def expected_links(setting, delta):
    """(kept rows, summary, links, info) of the model on the oracle's rows."""
    c = bp.planted()
    return pair_links(c["want"], M, *setting, delta, c["n_pairs"])


def index_of(kept, key):
    """The index of the kept row (qid, seq, pos)."""
    hit = np.flatnonzero((kept[:, 0] == key[0]) & (kept[:, 1] == key[1]) & (kept[:, 2] == key[2]))
    assert len(hit) == 1, key
    return int(hit[0])


def pair_mapq(kept, links, P):
    """The MAPQ that pair P's primary records carry (both the same)."""
    mine = np.flatnonzero(((kept[:, 0] >> np.uint64(2)) == P) & ((links["flags"] & PRIMARY) != 0))
    assert len(mine) == 2 and links["mapq"][mine[0]] == links["mapq"][mine[1]], P
    return int(links["mapq"][mine[0]])


@functools.lru_cache(maxsize=None)
def check():
    c = bp.check()
    by = {}
    for e in c["plan"]:
        by.setdefault(e["kind"], []).append(e)
    for setting in SETTINGS:
        for delta in DELTAS:
            kept, summary, links, info = expected_links(setting, delta)
            assert np.array_equal(kept, bp.expected(setting, delta)[0])
            assert np.array_equal(summary, bp.expected(setting, delta)[1])
    # "tie": one forward record, two reverse ones at the best total
    e, = by["tie"]
    for delta in (0, 1):
        kept, summary, links, info = expected_links(WIDE, delta)
        assert info["n_best"][e["pair"]] == 2 and pair_mapq(kept, links, e["pair"]) == 1
    # "copy+1": the dearer copy is the next placement, one error away, whatever delta keeps
    e, = by["copy+1"]
    for delta in (0, 1):
        kept, summary, links, info = expected_links(WIDE, delta)
        assert info["n_best"][e["pair"]] == 1 and pair_mapq(kept, links, e["pair"]) == 10, delta
    # "lone": no next placement
    e, = by["lone"]
    kept, summary, links, info = expected_links(WIDE, 0)
    assert pair_mapq(kept, links, e["pair"]) == 60
    # "shared" at delta 1: D sees A and A2 at the same cost and takes the smaller position, A, whose mate is
    # the cheaper B: D -> A, A -> B is a link that is not mutual; A2's only mate is D
    e, = by["shared"]
    kept, summary, links, info = expected_links(WIDE, 1)
    A, A2 = (index_of(kept, (4 * e["pair"], 0, e[k])) for k in ("a", "a2"))
    B, D = (index_of(kept, (4 * e["pair"] + 3, 0, e[k])) for k in ("b", "dear"))
    assert A + links["mate"][A] == B and B + links["mate"][B] == A
    assert links["flags"][A] == PRIMARY and links["flags"][B] == PRIMARY
    assert links["flags"][A2] == 0 and links["flags"][D] == 0
    assert D + links["mate"][D] == A and A2 + links["mate"][A2] == D
    assert not info["mutual"][D] and info["mutual"][A] and info["mutual"][B]
    # tandem runs: mate ranges across several 64-record blocks and a 256-thread workgroup; every shift ties
    kept, summary, links, info = expected_links(WIDE, 0)
    pair_of = (kept[:, 0] >> np.uint64(2)).astype(np.int64)
    for e in by["tandem"]:  # (two kept records: the exact place among some 200 rows of dearer shifts)
        assert info["range"][pair_of == e["pair"]].max() > 2 * 64, e
        assert info["n_best"][e["pair"]] == 1 and pair_mapq(kept, links, e["pair"]) == 10, e
    for e in by["tandem tie"]:
        assert info["range"][pair_of == e["pair"]].max() > 256 + 64, e
        assert info["n_best"][e["pair"]] >= 3 and pair_mapq(kept, links, e["pair"]) == 0, e
    # so that the case cannot silently stop covering them (WIDE, delta 0: 412 kept records with tied
    # mates, 559 links that are not mutual, ranges of up to 1013 rows)
    assert info["tied"].sum() >= 400, info["tied"].sum()
    assert (~info["mutual"]).sum() >= 500, (~info["mutual"]).sum()
    assert info["range"].max() >= 1000, info["range"].max()
    return c
