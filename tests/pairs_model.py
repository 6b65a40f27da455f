"""The pair rule (docs/semantics.md "Pairs") in numpy over sorted rows: the
checker of the device stage (sahara_amd/csrc/pairs.hip). Shares no code with
csrc/pairs_core.h."""
import numpy as np


def _keep(rows, length, min_fragment, max_fragment):
    if not 0 <= min_fragment <= max_fragment:
        raise ValueError("min_fragment must be in [0, max_fragment]")
    if max_fragment < length:
        raise ValueError("max_fragment is below the pattern length")
    dmin, dmax = max(min_fragment, length) - length, max_fragment - length
    q, s, p = (rows[:, i].astype(np.int64) for i in range(3))  # (positions are far below 2^62: signed sums do not wrap)
    # rows are sorted by (qid, seq_id, pos, err): the rows of one (qid, seq_id) are a run
    change = np.ones(len(rows), bool)
    change[1:] = (q[1:] != q[:-1]) | (s[1:] != s[:-1])
    first = np.flatnonzero(change)
    last = np.append(first[1:], len(rows))
    runs = {(int(q[a]), int(s[a])): (a, b) for a, b in zip(first.tolist(), last.tolist())}
    keep = np.zeros(len(rows), bool)
    for (qid, seq), (a, b) in runs.items():
        mate = runs.get((qid ^ 3, seq))
        if mate is None:
            continue
        there = np.unique(p[mate[0]:mate[1]])  # the partner's positions on this record, ascending
        here = p[a:b]
        # an even qid is the forward mate at a: its mates lie at b with dmin <= b - a <= dmax;
        # an odd qid is the reverse mate at b: the forward mates lie at a = b - d
        lo, hi = (here + dmin, here + dmax) if qid % 2 == 0 else (here - dmax, here - dmin)
        j = np.searchsorted(there, lo, side="left")
        keep[a:b] = (j < len(there)) & (there[np.minimum(j, len(there) - 1)] <= hi)
    return keep


def pairs(rows, length, min_fragment, max_fragment):
    """rows: (n, 4) of (qid, seq_id, pos, err) in canonical order, the reads
    interleaved as mate pairs with their reverse complements (pair p: qids 4p,
    4p + 1, 4p + 2, 4p + 3; the partner of q is q ^ 3). The rows that have a
    concordant mate among `rows`: same seq_id, the even qid's pos a and the
    odd one's pos b with max(min_fragment, length) <= b + length - a <=
    max_fragment. Order is kept."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    return rows[_keep(rows, length, min_fragment, max_fragment)]


def pair_count(rows):
    """The pairs that own a row."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    return len(np.unique(rows[:, 0] >> np.uint64(2)))
