"""The alignment rule of docs/semantics.md ("Alignments") as a plain banded DP
plus traceback: the checker of the device kernel (sahara_amd/csrc/align.hip).

Symbols are ranks; the text is the concatenated text of the index, every
record followed by one '$' (rank 0). Only the band |j - i| <= K of the cost
table is computed (a cell outside it costs more than K), so a 100-symbol hit
costs about a millisecond.
"""
from __future__ import annotations

INF = 1 << 30
NONE = 0xFFFFFFFF
MAX_ERR = 8
KIND_X, KIND_I, KIND_D = 1, 2, 3
_OPS = {KIND_X: "X", KIND_I: "I", KIND_D: "D"}


def concat_text(records):
    """The index's text: each record's ranks followed by one 0 ('$')."""
    out = []
    for r in records:
        out.extend(int(x) for x in r)
        out.append(0)
    return out


def window(T, g, m, K, edit):
    """JM: text symbols from g up to the first '$' or the text's end, capped at m + K (edit off: m)."""
    cap = m + K if edit else m
    j = 0
    while j < cap and g + j < len(T) and T[g + j] != 0:
        j += 1
    return j


def cost_table(P, T, g, K, edit):
    """(get, JM): get(i, j) = D[i][j] inside the band and the window, INF elsewhere."""
    m = len(P)
    JM = window(T, g, m, K, edit)
    B = K if edit else 0
    rows = [[INF] * (2 * B + 1) for _ in range(m + 1)]

    def get(i, j):
        if i < 0 or i > m or j < 0 or j > JM or abs(j - i) > B:
            return INF
        return rows[i][j - i + B]

    rows[0][B] = 0  # D[0][0]; D[0][j > 0] stays INF: a D can never be first
    for i in range(1, m + 1):
        for j in range(max(0, i - B), min(JM, i + B) + 1):
            best = INF
            if j > 0:  # = / X
                best = get(i - 1, j - 1) + (0 if P[i - 1] == T[g + j - 1] else 1)
            if edit:  # I: a pattern symbol with no text symbol
                best = min(best, get(i - 1, j) + 1)
            if edit and 0 < i < m and j > 0:  # D: a text symbol with no pattern symbol, never last
                best = min(best, get(i, j - 1) + 1)
            rows[i][j - i + B] = min(best, INF)
    return get, JM


def align(P, T, g, K, edit=True):
    """(err, ref_len, edits) of pattern P at text position g, or None (SAHARA_ALIGN_NONE).

    edits: (qpos, kind) in pattern order, qpos = pattern symbols before the edit.
    """
    m = len(P)
    get, JM = cost_table(P, T, g, K, edit)
    B = K if edit else 0
    ends = [(get(m, j), abs(j - m), j) for j in range(max(0, m - B), min(JM, m + B) + 1)]
    ends = [x for x in ends if x[0] <= K]
    if not ends:
        return None
    e_star = min(x[0] for x in ends)
    _, _, ref_len = min(x for x in ends if x[0] == e_star)  # closest to m, ties to the smaller j
    edits = []
    i, j = m, ref_len
    while i > 0 or j > 0:
        c = get(i, j)
        if i > 0 and j > 0:
            sub = 0 if P[i - 1] == T[g + j - 1] else 1
            if get(i - 1, j - 1) + sub == c:
                if sub:
                    edits.append((i - 1, KIND_X))
                i, j = i - 1, j - 1
                continue
        if edit and i > 0 and get(i - 1, j) + 1 == c:
            edits.append((i - 1, KIND_I))
            i -= 1
            continue
        if edit and 0 < i < m and j > 0 and get(i, j - 1) + 1 == c:
            edits.append((i, KIND_D))
            j -= 1
            continue
        raise AssertionError("traceback stuck at (%d, %d)" % (i, j))
    edits.reverse()
    assert len(edits) == e_star
    return e_star, ref_len, edits


def apply(P, T, g, ref_len, edits):
    """Replays a record: True iff the edits turn T[g, g + ref_len) into P without touching a '$'."""
    m = len(P)
    i = j = 0

    def matches(upto):
        nonlocal i, j
        while i < upto:
            if g + j >= len(T) or T[g + j] == 0 or P[i] != T[g + j]:
                return False
            i += 1
            j += 1
        return True

    for qpos, kind in edits:
        if qpos < i or qpos > m or not matches(qpos):
            return False
        if kind == KIND_X:
            if i >= m or g + j >= len(T) or T[g + j] == 0 or P[i] == T[g + j]:
                return False
            i += 1
            j += 1
        elif kind == KIND_I:
            if i >= m:
                return False
            i += 1
        elif kind == KIND_D:
            if g + j >= len(T) or T[g + j] == 0:
                return False
            j += 1
        else:
            return False
    return matches(m) and j == ref_len


def cigar(edits, m):
    """Extended CIGAR of a record's edits: runs of '=' between them, equal neighbours merged."""
    ops = []
    i = 0
    for qpos, kind in edits:
        ops.extend("=" * (qpos - i))
        i = qpos
        ops.append(_OPS[kind])
        if kind != KIND_D:
            i += 1
    ops.extend("=" * (m - i))
    out = []
    k = 0
    while k < len(ops):
        r = k
        while r < len(ops) and ops[r] == ops[k]:
            r += 1
        out.append("%d%s" % (r - k, ops[k]))
        k = r
    return "".join(out)


def record_of(res):
    """A model result in the fields of sahara_alignment: (err, ref_len, [edit words])."""
    if res is None:
        return NONE, 0, [0] * MAX_ERR
    e, ref_len, edits = res
    words = [(q << 2) | k for q, k in edits]
    return e, ref_len, words + [0] * (MAX_ERR - len(words))
