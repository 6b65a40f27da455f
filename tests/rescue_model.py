"""The mate rescue (docs/semantics.md "Mate rescue") over sorted rows: the
checker of the device stage (sahara_amd/csrc/rescue.hip). Shares no code with
csrc/rescue_core.h or csrc/align_core.h: one anchor's scan is the oracle's
brute-force DP over the window cut out of its record."""
import numpy as np

import oracle as O
from pairs_model import _keep

MAX_WINDOW = 4096


def window(qid, pos, dmin, dmax, rec_len):
    """The starts [lo, hi] on the hit's record where its partner is looked for, or None."""
    if qid % 2 == 0:
        lo, hi = pos + dmin, pos + dmax
    else:
        if pos < dmin:
            return None
        lo, hi = max(pos - dmax, 0), pos - dmin
    if rec_len == 0 or lo > rec_len - 1:
        return None
    return lo, min(hi, rec_len - 1)


_SCANS = {}  # (the same windows come back for every K, batch size and entry point of the tests)


def scan(rec, pat, lo, hi, K, edit):
    """The least (e*, start) over the starts [lo, hi] of `rec` for `pat` within
    K errors, or None: the brute force over rec[lo : hi + len + K] as a record
    of its own, its rows at most hi - lo from the cut's start."""
    pat = np.ascontiguousarray(pat, dtype=np.uint8)
    cut = np.ascontiguousarray(rec[lo:min(hi + len(pat) + K, len(rec))], dtype=np.uint8)
    key = (cut.tobytes(), pat.tobytes(), K, bool(edit), hi - lo)
    if key not in _SCANS:
        rows = O.bruteforce([cut], pat[None, :], K, edit=edit)
        rows = rows[rows[:, 2] <= hi - lo]
        _SCANS[key] = min(((int(r[3]), int(r[2])) for r in rows), default=None)
    got = _SCANS[key]
    return None if got is None else (got[0], lo + got[1])


def anchors(rows, recs, length, min_fragment, max_fragment, A):
    """(indices of the anchors of `rows` that are scanned, queries the cap left alone)."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    dmin, dmax = max(min_fragment, length) - length, max_fragment - length
    keep = _keep(rows, length, min_fragment, max_fragment)
    per = {}
    for i in range(len(rows)):
        q, s, p = (int(v) for v in rows[i, :3])
        if keep[i] or (i and (rows[i, :3] == rows[i - 1, :3]).all()):
            continue
        if window(q, p, dmin, dmax, len(recs[s])) is None:
            continue
        per.setdefault(q, []).append(i)
    capped = [q for q, v in per.items() if A and len(v) > A]
    idx = sorted(i for q, v in per.items() if not (A and len(v) > A) for i in v)
    return idx, capped


def rescue(rows, pats, recs, length, min_fragment, max_fragment, K, edit=True, A=0, stats=None):
    """rows: (n, 4) of (qid, seq_id, pos, err) in canonical order, as the pair
    stage takes them; pats: the interleaved patterns (qid -> ranks); recs: the
    records. Returns the rows of H u R in canonical order. stats (a dict):
    gets anchors, capped_queries, starts and rescued."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 4)
    if not 1 <= K <= 8:
        raise ValueError("K must be in [1, 8]")
    dmin, dmax = max(min_fragment, length) - length, max_fragment - length
    if dmax - dmin >= MAX_WINDOW:
        raise ValueError("the fragment window is too wide")
    idx, capped = anchors(rows, recs, length, min_fragment, max_fragment, A)
    found, starts = set(), 0
    for i in idx:
        q, s, p = (int(v) for v in rows[i, :3])
        lo, hi = window(q, p, dmin, dmax, len(recs[s]))
        starts += hi - lo + 1
        got = scan(recs[s], pats[q ^ 3], lo, hi, K, edit)
        if got is not None:
            found.add((q ^ 3, s, got[1], got[0]))
    if stats is not None:
        stats.update(anchors=len(idx), capped_queries=len(capped), starts=starts, rescued=len(found))
    if not found:
        return rows
    out = np.concatenate([rows, np.array(sorted(found), np.uint64).reshape(-1, 4)])
    return out[np.lexsort((out[:, 3], out[:, 2], out[:, 1], out[:, 0]))]
