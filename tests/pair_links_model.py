"""The pair-links rule (docs/semantics.md "Pair links") in numpy and Python
over sorted rows, on top of tests/best_pairs_model.py: the checker of the pair
stage's links (sahara_amd/csrc/pairs.hip). Shares no code with csrc/."""
import numpy as np

from best_pairs_model import NONE, best_pairs, scores

LINK_DTYPE = np.dtype([("mate", "<i4"), ("score", "u1"), ("mapq", "u1"), ("flags", "u1"), ("reserved", "u1")])
PRIMARY = 1


def mapq(best, nxt, n_best):
    """The pair's MAPQ: a policy. n_best: the larger of its kept even-qid and
    kept odd-qid records with m == best."""
    if best == NONE or n_best == 0:
        return 0
    if n_best >= 3:
        return 0
    if n_best == 2:
        return 1
    gap = 6 if nxt == NONE else min(nxt - best, 6)
    return 10 * gap


def pair_links(rows, length, min_fragment, max_fragment, delta, n_pairs=None):
    """rows as best_pairs takes them. Returns (kept_rows, summary, links,
    info): best_pairs' two, one LINK_DTYPE record per kept row, and what the
    tests ask about the case: per kept row `range` (the rows of R(i)), `tied`
    (R(i) holds its least err more than once) and `mutual`; per pair `n_best`
    and `mapq`. Asserts what the rule promises: the mate of a kept record is
    kept and of its pair, a pair's primary even-qid record has the score best
    and a mutual link."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    kept_rows, summary = best_pairs(rows, length, min_fragment, max_fragment, delta, n_pairs)
    n_pairs = len(summary)
    m = scores(rows, length, min_fragment, max_fragment)
    dmin, dmax = max(min_fragment, length) - length, max_fragment - length
    q, s, p, e = (rows[:, i].astype(np.int64) for i in range(4))
    pair = q >> 2
    head = np.ones(len(rows), bool)
    head[1:] = (rows[1:, :3] != rows[:-1, :3]).any(axis=1)
    best = summary["best"].astype(np.int64)
    keep = head & (m != NONE) & (m <= best[pair] + delta)
    assert np.array_equal(rows[keep], kept_rows)
    change = np.ones(len(rows), bool)
    change[1:] = (q[1:] != q[:-1]) | (s[1:] != s[:-1])
    first = np.flatnonzero(change)
    runs = {(int(q[a]), int(s[a])): (a, b) for a, b in zip(first.tolist(), np.append(first[1:], len(rows)).tolist())}
    kept = np.flatnonzero(keep)
    new = np.cumsum(keep) - 1  # a kept row's index among the kept ones
    mate = np.full(len(rows), -1, np.int64)
    size = np.zeros(len(rows), np.int64)
    tied = np.zeros(len(rows), bool)
    for i in kept.tolist():
        a, b = runs[(int(q[i]) ^ 3, int(s[i]))]
        lo, hi = (p[i] + dmin, p[i] + dmax) if q[i] % 2 == 0 else (p[i] - dmax, p[i] - dmin)
        jl = a + int(np.searchsorted(p[a:b], lo, side="left"))
        jr = a + int(np.searchsorted(p[a:b], hi, side="right"))
        assert jl < jr
        least = int(e[jl:jr].min())
        j = jl + int(np.flatnonzero(e[jl:jr] == least)[0])  # the least err, ties to the smaller index
        assert e[i] + e[j] == m[i]
        assert head[j], "the mate is the first record of its position"
        assert keep[j], "the mate of a kept record is kept"
        mate[i], size[i], tied[i] = j, jr - jl, (e[jl:jr] == least).sum() > 1
    primary = np.zeros(len(rows), bool)
    n_best = np.zeros(n_pairs, np.int64)
    pair_mapq = np.zeros(n_pairs, np.int64)
    odd = (q & 1).astype(bool)
    for P in np.unique(pair[kept]).tolist():
        mine = kept[pair[kept] == P]
        even = mine[~odd[mine]]
        assert len(even) and len(mine) > len(even), "a pair keeps records of both reads or of neither"
        star = int(even[np.lexsort((even, m[even]))[0]])  # the least (m, canonical index)
        assert m[star] == best[P]
        assert mate[mate[star]] == star, "the primary link is mutual"
        primary[star] = primary[mate[star]] = True
        n_best[P] = max(int((m[even] == best[P]).sum()), int((m[mine[odd[mine]]] == best[P]).sum()))
        pair_mapq[P] = mapq(int(summary["best"][P]), int(summary["next"][P]), int(n_best[P]))
    links = np.zeros(len(kept), LINK_DTYPE)
    links["mate"] = new[mate[kept]] - new[kept]
    links["score"] = m[kept]
    links["flags"] = np.where(primary[kept], PRIMARY, 0)
    links["mapq"] = np.where(primary[kept], pair_mapq[pair[kept]], 0)
    at = np.arange(len(kept))
    there = at + links["mate"]
    assert ((there >= 0) & (there < len(kept))).all()
    assert (kept_rows[there, 0] == (kept_rows[:, 0] ^ np.uint64(3))).all()  # the mate is of the partner qid: same pair
    mutual = (there + links["mate"][there]) == at
    info = dict(range=size[kept], tied=tied[kept], mutual=mutual, n_best=n_best, mapq=pair_mapq)
    return kept_rows, summary, links, info
