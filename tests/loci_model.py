"""The loci rule (docs/semantics.md "Loci") as a sequential scan over sorted
rows: the checker of the device stage (sahara_amd/csrc/loci.hip). Shares no
code with csrc/loci_core.h."""
import numpy as np


def loci(rows, W):
    """rows: (n, 4) of (qid, seq_id, pos, err) in canonical order. One row per
    locus: a locus is a maximal run of one query's positions in one record in
    which each distinct position is at most W above the one before; its row is
    the one with the least err, ties to the smaller pos. Order is kept."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    out = []
    best = None  # the current locus's representative so far
    prev = None  # the row before
    for q, s, p, e in rows.tolist():
        new = prev is None or q != prev[0] or s != prev[1] or p - prev[2] > W
        if new:
            if best is not None:
                out.append(best)
            best = (q, s, p, e)
        elif e < best[3]:  # strictly: on a tie the earlier row (smaller pos) stays
            best = (q, s, p, e)
        prev = (q, s, p, e)
    if best is not None:
        out.append(best)
    return np.array(out, np.uint64).reshape(-1, 4)


def locus_ids(rows, W):
    """Per row the number of its locus (0, 1, ...), by the same scan."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    ids, cur, prev = [], -1, None
    for q, s, p, _ in rows.tolist():
        if prev is None or q != prev[0] or s != prev[1] or p - prev[2] > W:
            cur += 1
        ids.append(cur)
        prev = (q, s, p)
    return np.array(ids, np.int64)
