"""The planted text (tests/planted.py) against the oracle, and the properties
its query layouts exist for, without a GPU: what lets
tests/test_hit_chain_edges.py take the construction as its expectation."""
import functools

import numpy as np
import pytest

import oracle as O
import planted as P
from helpers import hits_as_rows
from test_golden import limit_rows


@functools.lru_cache(maxsize=None)
def _oracle(sigma, nrec):
    return O.Index.build(P.build(sigma, nrec).records, sigma, 16)


def _ham(k):
    return O.scheme("h2-k2", 0, k, P.M, hamming=True)


def test_text_shape():
    t5, t300 = P.build(6, 5), P.build(6, 300)
    assert len(t5.records) == 5 and len(t300.records) == 300  # 300: record starts past the LDS table of 256
    assert np.array_equal(np.concatenate(t5.records), np.concatenate(t300.records))
    assert 400_000 < t5.n_symbols < 600_000
    for c in P.COUNTS:
        t = t5.table[c]
        assert (t[:, 2] == 0).sum() == c and (t[:, 2] == 1).sum() == P.SUBS.get(c, 0)
    for c0, c1 in P.LIMIT_PAIRS:
        assert P.SUBS[c0] == c1
    d4 = P.build(5, 5)
    assert max(r.max() for r in d4.records) == 4 and max(r.max() for r in t5.records) == 5
    assert not any((r == 4).any() for r in t5.records)  # no N


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("nrec", [5, 300])
@pytest.mark.parametrize("sigma", [6, 5])
def test_construction_equals_oracle(sigma, nrec, k):
    """Every distinct count queried once plus every random pattern, Hamming
    k: the oracle's sorted rows are the construction's rows as emitted."""
    t = P.build(sigma, nrec)
    layout = list(P.COUNTS) + [0] * P.N_RANDOM
    zeros = t.patterns(layout)[len(P.COUNTS):]
    assert len(np.unique(zeros, axis=0)) == P.N_RANDOM  # consecutive zeros take all the random patterns
    want = hits_as_rows(_oracle(sigma, nrec).search(t.patterns(layout), _ham(k), edit=False, nthreads=8)[0])
    got = t.expected(layout, k)
    assert len(got) == sum(P.COUNTS) + (sum(P.SUBS.values()) if k else 0)
    assert np.array_equal(got, want)
    assert np.array_equal(hits_as_rows(got), got)  # emitted in canonical order already
    assert np.array_equal(t.per_query(layout, 0), layout)


def test_expected_of_repeated_and_offset_queries():
    """expected() over a layout with repeats is the single-query blocks back to back."""
    t = P.build(6, 5)
    layout = [9, 0, 3, 9, 65, 0, 3]
    e = t.expected(layout, 1, qid0=100)
    parts = []
    for i, c in enumerate(layout):
        b = t.block(c, 1)
        parts.append(np.column_stack([np.full(len(b), 100 + i, np.uint64), b]).reshape(-1, 4))
    assert np.array_equal(e, np.concatenate(parts))
    pats = t.patterns(layout)
    assert np.array_equal(pats[0], pats[3]) and not np.array_equal(pats[1], pats[5])


def _sums(layout):
    a = np.asarray(layout)
    return a.reshape(-1, P.RANGE).sum(1)


def test_layout_a_ranges():
    R = P.RANGES_A
    assert all(len(r) == P.RANGE for r in R.values())
    assert len(P.LAYOUT_A) == P.RANGE * len(R)
    # every tier edge in one range that fits the tile exactly, and its twin one row past it
    for name, total in (("edges_1024", P.TILE), ("edges_1025", P.TILE + 1)):
        r = R[name]
        assert sum(r) == total
        for c in (0, 1, P.SMALL, P.SMALL + 1, P.MEDIUM - 1, P.MEDIUM, P.MEDIUM + 1, 10):
            assert c in r
        assert [P.tier(c) for c in (8, 9, 64, 65)] == ["small", "medium", "medium", "long"]
        assert sum(1 for c in r if c > P.MEDIUM) == 1  # one skipped segment
    assert sum(R["256x4"]) == P.TILE and set(R["256x4"]) == {4}
    assert R["1024_alone"][0] == 1024 and sum(R["1024_alone"]) == P.TILE  # every row of the tile skipped
    assert sum(R["16x64"]) == P.TILE and R["16x64"].count(64) == 16
    for name in ("wave_medium", "wave_medium_global"):
        wave1 = R[name][64:128]
        assert all(P.tier(c) == "medium" for c in wave1) and set(wave1) == {9, 10}
    assert sum(R["wave_medium"]) <= P.TILE < sum(R["wave_medium_global"])
    names = list(R)
    z = names.index("zeros")
    assert sum(R["zeros"]) == 0 and sum(R[names[z - 1]]) == P.TILE == sum(R[names[z + 1]])
    # the layout's hit counts are its numbers (Hamming, k = 0)
    assert np.array_equal(P.build(6, 5).per_query(P.LAYOUT_A, 0), P.LAYOUT_A)


def test_layout_b_places():
    for lay in (P.LAYOUT_B1, P.LAYOUT_B2):
        assert set(P.LONG_COUNTS) <= set(lay) and len(lay) > P.RANGE
        first, last, left, right = lay[0], lay[-1], lay[P.RANGE - 1], lay[P.RANGE]
        assert {P.tier(first), P.tier(last)} == {"long", "huge"}
        assert {P.tier(left), P.tier(right)} == {"long", "huge"}
    assert P.tier(P.LAYOUT_B1[0]) == "long" and P.tier(P.LAYOUT_B2[0]) == "huge"
    assert P.LAYOUT_B2[P.RANGE - 1] == P.LDS  # the last size sorted in LDS, at a range's end
    assert [P.tier(c) for c in (2048, 2049)] == ["long", "huge"]


@pytest.mark.parametrize("nq", P.NQ_EDGES)
def test_layout_c_ends_long(nq):
    lay = P.layout_c(nq)
    assert len(lay) == nq and P.tier(lay[-1]) == "long"
    if nq > 2:
        assert P.tier(lay[-2]) == "huge"
    # the scan works on nq + 1 counts: at 4095 the sentinel is a tile's last
    # element, at 4096 it is alone in the second tile
    assert (nq + 1 + P.SCAN_TILE - 1) // P.SCAN_TILE == (1 if nq < P.SCAN_TILE else 2)


def test_layout_d_passes_one_scan_trip():
    lay = P.layout_d()
    assert len(lay) == P.NQ_D > P.ONE_TRIP == 1 << 20
    tiles = (len(lay) + 1 + P.SCAN_TILE - 1) // P.SCAN_TILE
    assert tiles == 257  # the smallest count of tiles at which the second trip runs
    tail = lay[P.ONE_TRIP:]
    assert 65 in tail and 2049 in tail and lay[:P.ONE_TRIP].max() <= P.SMALL
    assert lay[:P.ONE_TRIP].sum() > 0  # a carried sum of zero would hide a lost carry
    rows = int(lay.sum())
    assert 1_500_000 < rows < 1_650_000
    t = P.build(6, 5)
    e = t.expected(lay, 0)
    assert len(e) == rows and np.array_equal(np.bincount(e[:, 0].astype(np.int64), minlength=len(lay)), lay)


def test_layout_e_passes_each_cap():
    longs = lambda lay: sum(1 for c in lay if P.tier(c) == "long")  # noqa: E731
    assert longs(P.LAYOUT_E_65) > P.BIG_LDS_GRID and set(P.LAYOUT_E_65) == {65}
    assert longs(P.LAYOUT_E_MIXED) > P.BIG_LDS_GRID and set(P.LAYOUT_E_MIXED) == {65, 2048}
    assert P.LAYOUT_E_LLIST[:P.SCAN_TILE] == [65] * P.SCAN_TILE  # every query of the first scan tile is long
    assert P.CAP_8192 < sum(P.LAYOUT_E_2M) < P.CAP_16384 < sum(P.LAYOUT_E_4M)
    assert sum(P.LAYOUT_E_2M) - P.CAP_8192 > 4097  # whole queries lie past the cap
    # the strided trip of a kSortBigLds workgroup (list entry s + 4096) meets both lengths
    assert {65, 2048} <= set(P.LAYOUT_E_MIXED[P.BIG_LDS_GRID:])
    assert (P.LAYOUT_E_MIXED[7], P.LAYOUT_E_MIXED[7 + P.BIG_LDS_GRID]) == (2048, 65)
    assert (P.LAYOUT_E_MIXED[4], P.LAYOUT_E_MIXED[4 + P.BIG_LDS_GRID]) == (65, 2048)


def test_layout_e_parts_passes_the_cap_in_one_part():
    """kOffsetSeq sees one part's hits at a time: the three-part case has a
    part whose hits alone pass 8192 x 256, the merged total passes it for
    kQidKeys and kGatherHits, and the smaller case (compact, fetch, digest)
    would not do for kOffsetSeq."""
    t = P.build(6, 5)
    assert P.split_records(t.records) == [0, 2, 4, 5]
    per = P.hits_per_part(t, P.LAYOUT_E_PARTS)
    assert per.sum() == sum(P.LAYOUT_E_PARTS) == len(P.LAYOUT_E_PARTS) * 4097
    assert per.max() > P.CAP_8192 + 4097
    assert P.hits_per_part(t, P.LAYOUT_E_2M).max() < P.CAP_8192
    for nq in P.NQ_PARTS:  # the merge cases have rows in every part
        assert (P.hits_per_part(t, P.layout_g(nq)) > 0).all()


def test_layout_g_counts():
    for nq in P.NQ_PARTS:
        lay = P.layout_g(nq)
        assert len(lay) == nq and lay[0] == P.LONG_COUNTS[0]
    # pattern counts at a power of two and one past it (sortHitsByQid's endBit)
    assert {1, 2, 3, 4, 5, 1024, 1025} == set(P.NQ_PARTS)


def test_limit_cases_hit_their_branches():
    """limit_rows over the construction equals the same over the oracle's
    rows for every n of the quota cases, and each case is in the branch it is
    named for."""
    t = P.build(6, 5)
    layout = [c0 for c0, _ in P.LIMIT_PAIRS]
    want = hits_as_rows(_oracle(6, 5).search(t.patterns(layout), _ham(1), edit=False, nthreads=8)[0])
    got = t.expected(layout, 1)
    assert np.array_equal(got, want)
    cases = P.limit_cases()
    assert {b for *_, b in cases} == {"all kept", "ends at level 0", "cut inside level 0", "cut inside level 1"}
    for n in sorted({n for _, _, n, _ in cases}):
        assert np.array_equal(limit_rows(got, n), limit_rows(want, n))
    for c0, c1, n, branch in cases:
        rows = t.expected([c0], 1)
        hist = np.bincount(rows[:, 3].astype(np.int64), minlength=2)
        assert list(hist) == [c0, c1]
        distinct = len(rows)
        kept = limit_rows(rows, n)
        if branch == "all kept":
            assert distinct <= n and len(kept) == distinct
        elif branch == "ends at level 0":
            assert distinct > n == hist[0] and (kept[:, 3] == 0).all() and len(kept) == n
        elif branch == "cut inside level 0":
            assert n < hist[0] and (kept[:, 3] == 0).all() and len(kept) == n
        else:
            assert hist[0] < n < distinct and (kept[:, 3] == 1).sum() == n - c0 and len(kept) == n
