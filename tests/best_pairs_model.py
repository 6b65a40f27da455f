"""The best-pairs rule (docs/semantics.md "Best pairs") in numpy over sorted
rows: the checker of the pair stage's best mode (sahara_amd/csrc/pairs.hip).
Shares no code with csrc/best_pairs_core.h or csrc/pairs_core.h."""
import numpy as np

NONE = 255  # a score without a value; the summary's "keeps nothing" / "no next"
SUMMARY_DTYPE = np.dtype([("best", "u1"), ("next", "u1"), ("n_fwd", "<u2"), ("n_rev", "<u2"), ("reserved", "<u2")])


def scores(rows, length, min_fragment, max_fragment, counts=None):
    """m(i) per row: its err plus the least err among the rows of its partner
    qid on its record within its fragment window; NONE where there is none.
    counts: an int array of len(rows) that receives the rows in each window."""
    if not 0 <= min_fragment <= max_fragment:
        raise ValueError("min_fragment must be in [0, max_fragment]")
    if max_fragment < length:
        raise ValueError("max_fragment is below the pattern length")
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    dmin, dmax = max(min_fragment, length) - length, max_fragment - length
    q, s, p, e = (rows[:, i].astype(np.int64) for i in range(4))
    change = np.ones(len(rows), bool)
    change[1:] = (q[1:] != q[:-1]) | (s[1:] != s[:-1])
    first = np.flatnonzero(change)
    last = np.append(first[1:], len(rows))
    runs = {(int(q[a]), int(s[a])): (a, b) for a, b in zip(first.tolist(), last.tolist())}
    m = np.full(len(rows), NONE, np.int64)
    for (qid, seq), (a, b) in runs.items():
        mate = runs.get((qid ^ 3, seq))
        if mate is None:
            continue
        there, cost = p[mate[0]:mate[1]], e[mate[0]:mate[1]]  # the partner's positions, ascending, and their errs
        here = p[a:b]
        lo, hi = (here + dmin, here + dmax) if qid % 2 == 0 else (here - dmax, here - dmin)
        jl = np.searchsorted(there, lo, side="left")
        jr = np.searchsorted(there, hi, side="right")
        if counts is not None:
            counts[a:b] = jr - jl
        least = np.full(b - a, NONE, np.int64)
        for v in sorted(set(cost.tolist()), reverse=True):  # the smallest err present in [jl, jr) is written last
            upto = np.concatenate(([0], np.cumsum(cost == v)))
            least[upto[jr] > upto[jl]] = v
        m[a:b] = np.where(least == NONE, NONE, e[a:b] + least)
    return m


def best_pairs(rows, length, min_fragment, max_fragment, delta, n_pairs=None):
    """rows: (n, 4) of (qid, seq_id, pos, err) in canonical order (pair P owns
    the qids 4P .. 4P + 3). Returns (kept_rows, summary): the rows that are the
    first of their (qid, seq_id, pos), have a score and lie within `delta` of
    their pair's least score, in order; and one SUMMARY_DTYPE record per pair
    0 .. n_pairs - 1 (default: up to the last pair that owns a row)."""
    if not 0 <= delta <= 30:
        raise ValueError("delta must be in [0, 30]")
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    pair = (rows[:, 0] >> np.uint64(2)).astype(np.int64)
    if n_pairs is None:
        n_pairs = int(pair.max()) + 1 if len(rows) else 0
    m = scores(rows, length, min_fragment, max_fragment)
    head = np.ones(len(rows), bool)
    head[1:] = (rows[1:, :3] != rows[:-1, :3]).any(axis=1)
    has = m != NONE
    best = np.full(n_pairs, NONE, np.int64)
    np.minimum.at(best, pair[has], m[has])
    keep = head & has & (m <= best[pair] + delta)
    other = head & has & (m > best[pair])
    nxt = np.full(n_pairs, NONE, np.int64)
    np.minimum.at(nxt, pair[other], m[other])
    summary = np.zeros(n_pairs, SUMMARY_DTYPE)
    summary["best"], summary["next"] = best, nxt
    odd = (rows[:, 0] & np.uint64(1)).astype(bool)
    summary["n_fwd"] = np.minimum(np.bincount(pair[keep & ~odd], minlength=n_pairs), 65535)
    summary["n_rev"] = np.minimum(np.bincount(pair[keep & odd], minlength=n_pairs), 65535)
    return rows[keep], summary


def stats_of(kept, summary):
    """What sahara_best_pairs_stats reports beside hits_in: (kept, pairs, unique_pairs)."""
    return (len(kept), int((summary["best"] != NONE).sum()),
            int(((summary["n_fwd"] == 1) & (summary["n_rev"] == 1)).sum()))
