"""Batches of more than 8192 x 256 rows for the post-sort stages (loci, mate
rescue, pairs, --max_hits), with an exact expectation and no oracle run (CPU
only, numpy only). No GPU: tests/test_stage_caps_gpu.py runs the cases on one,
tests/test_stage_caps_case.py proves them first.

The text is tests/planted.py's. A *group* is four consecutive qids 4p .. 4p + 3
(one mate pair with its reverse complements; the partner of q is q ^ 3), and a
group *type* is the planted counts of its forward and its reverse mate,
(a, 0, 0, b): qid 4p is the unit u_a, qid 4p + 3 the unit u_b, the two between
find nothing (0 for a or b: a random pattern, which finds nothing either). All
stages act per query, per mate pair or per locus, and a locus, a pair and a
query never leave their group, so the rows of a batch of many groups are the
rows of each type's one group (the sequential models, run on that type's four
queries) tiled with the qid shifted by 4p, and the stages' figures are the
types' figures summed. Every group of a type has the same four patterns (a
random one is planted.random[its place in the group]), so this holds for the
rescue's scans too.

A *layout* is the list of its groups' types, in order. The layouts below pass
CAP = 8192 x 256 rows in one batch, which is where every per-hit kernel of
the stages starts its second grid-stride trip; what each is for is asserted
in tests/test_stage_caps_case.py.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import planted as P
from loci_model import loci, locus_ids
from pairs_model import _keep, pair_count
from rescue_model import anchors, rescue, scan, window
from test_golden import RC, limit_rows

SIGMA, M, CAP = 6, P.M, P.CAP_8192


def text():
    return P.build(SIGMA, 5)


class Stages(NamedTuple):
    """The stages of a call, in pass_plan.h's order: loci window W; the mate
    rescue (max_err, anchor cap; 0: none) in the pair window; pairs
    (min_fragment, max_fragment); --max_hits."""
    W: Optional[int] = None
    rescue: Optional[Tuple[int, int]] = None
    frag: Optional[Tuple[int, int]] = None
    limit: int = 0


# ------------------------------------------------------------ patterns ----

def rc(x):
    return RC[SIGMA][np.asarray(x, np.uint8)][..., ::-1]


def group_patterns(typ):
    """(4, M): the group's patterns as a caller of search() gives them."""
    t = text()
    assert len(typ) == 4 and typ[1] == 0 and typ[2] == 0  # (the packed entry points put reverse complements there)
    return np.stack([t.unit[c] if c else t.random[j] for j, c in enumerate(typ)])


def patterns(layout):
    tab = {typ: group_patterns(typ) for typ in set(layout)}
    return np.ascontiguousarray(np.concatenate([tab[typ] for typ in layout]))


def reads(layout):
    """(2 per group, M) for the entry points that add the reverse complements
    on the device: read 2p is qid 4p's pattern, read 2p + 1 the reverse
    complement of qid 4p + 3's."""
    p = patterns(layout)
    out = np.empty((2 * len(layout), M), np.uint8)
    out[0::2] = p[0::4]
    out[1::2] = rc(p[3::4])
    return out


def with_rc(r):
    """What the device searches for `reads`: qid 2i is read i, qid 2i + 1 its reverse complement."""
    out = np.empty((2 * len(r), r.shape[1]), np.uint8)
    out[0::2] = r
    out[1::2] = rc(r)
    return out


# ------------------------------------------------- one group of a type ----

def group_rows(typ, k):
    """Canonical rows of the type's one group (qids 0 .. 3) under Hamming k."""
    return text().expected(list(typ), k)


class Trace(NamedTuple):
    """One group through the stages. rows_in[s] are the rows stage s is given,
    mark[s] a flag per such row (below), out the call's rows, figures[s] what
    the stage reports."""
    rows_in: dict
    mark: dict
    out: np.ndarray
    figures: dict
    capped: tuple     # the rescue: qids (0 .. 3) the cap left alone
    uncapped: tuple   # qids with anchors that were scanned


def _heads_and_reps(rows, W):
    ids = locus_ids(rows, W)
    head = np.diff(ids, prepend=-1) != 0
    first = np.flatnonzero(head)
    last = np.append(first[1:], len(rows))
    rep = np.zeros(len(rows), bool)
    err = rows[:, 3].astype(np.int64)
    for a, b in zip(first.tolist(), last.tolist()):
        rep[a + int(np.argmin(err[a:b]))] = True  # (argmin: the first of the least)
    return head, rep, last - first


@functools.lru_cache(maxsize=None)
def trace(typ, k, st):
    t = text()
    rows = group_rows(typ, k)
    rows_in, mark, fig = {}, {}, {}
    capped = uncapped = ()
    if st.W is not None:
        out = loci(rows, st.W)
        head, rep, sizes = _heads_and_reps(rows, st.W)
        assert np.array_equal(rows[rep], out)
        # head: the row starts a locus; late: it is a representative and not its locus's first row
        rows_in["loci"], mark["loci"] = rows, dict(head=head, late=rep & ~head, sizes=sizes)
        fig["loci"] = dict(hits_in=len(rows), loci=len(out))
        rows = out
    if st.rescue is not None:
        Kr, A = st.rescue
        pats = group_patterns(typ)
        s = {}
        out = rescue(rows, pats, t.records, M, *st.frag, Kr, False, A, s)
        idx, cq = anchors(rows, t.records, M, *st.frag, A)
        dmin, dmax = max(st.frag[0], M) - M, st.frag[1] - M
        anchor = np.zeros(len(rows), bool)
        finds = np.zeros(len(rows), bool)
        for i in idx:
            q, r, p = (int(v) for v in rows[i, :3])
            anchor[i] = True
            finds[i] = scan(t.records[r], pats[q ^ 3], *window(q, p, dmin, dmax, len(t.records[r])), Kr, False) is not None
        # anchor: the row's window is scanned; finds: the scan finds the partner
        rows_in["rescue"], mark["rescue"] = rows, dict(anchor=anchor, finds=finds)
        fig["rescue"] = s
        capped = tuple(sorted(cq))
        uncapped = tuple(sorted({int(q) for q in rows[idx, 0]}))
        rows = out
    if st.frag is not None:
        keep = _keep(rows, M, *st.frag)
        out = rows[keep]
        rows_in["pairs"], mark["pairs"] = rows, dict(keep=keep)
        fig["pairs"] = dict(hits_in=len(rows), kept=len(out), pairs=pair_count(out))
        rows = out
    if st.limit:
        out = limit_rows(rows, st.limit) if len(rows) else rows
        per_q = np.bincount(rows[:, 0].astype(np.int64), minlength=4)
        rows_in["limit"], mark["limit"] = rows, dict(cut=(per_q > st.limit)[rows[:, 0].astype(np.int64)])
        rows = out
    return Trace(rows_in, mark, rows, fig, capped, uncapped)


# -------------------------------------------------------------- tiling ----

def _tile(layout, block, qid=True):
    """block(typ) -> array of the type's one group; the groups' arrays back
    to back, column 0 shifted by 4 x the group's number if `qid`."""
    types = list(dict.fromkeys(layout))
    number = {typ: i for i, typ in enumerate(types)}
    code = np.array([number[typ] for typ in layout], np.int64)
    blocks = [np.asarray(block(typ)) for typ in types]
    per = np.array([len(b) for b in blocks], np.int64)[code]
    off = np.concatenate([[0], np.cumsum(per)])
    out = np.empty((int(off[-1]),) + blocks[0].shape[1:], blocks[0].dtype)
    for i, b in enumerate(blocks):
        g = np.flatnonzero(code == i)
        if len(b) == 0 or len(g) == 0:
            continue
        dst = (off[g][:, None] + np.arange(len(b))[None, :]).ravel()
        out[dst] = np.tile(b, (len(g),) + (1,) * (b.ndim - 1))
        if qid:
            out[dst, 0] += np.repeat(4 * g, len(b)).astype(out.dtype)
    return out, off


class Expect(NamedTuple):
    rows: np.ndarray   # the call's rows, canonical order
    figures: dict      # stage -> the figures it reports, summed over the groups
    entering: dict     # stage -> the rows it is given


def expected(layout, k, stages):
    """What a call of the layout's patterns returns under Hamming k with `stages` on."""
    layout = list(layout)
    tr = {typ: trace(typ, k, stages) for typ in set(layout)}
    rows, _ = _tile(layout, lambda typ: tr[typ].out)
    count = {typ: layout.count(typ) for typ in tr}
    figures, entering = {}, {}
    for stage in ("loci", "rescue", "pairs", "limit"):
        if stage not in next(iter(tr.values())).rows_in:
            continue
        entering[stage] = sum(len(tr[typ].rows_in[stage]) * n for typ, n in count.items())
        if stage != "limit":
            names = next(iter(tr.values())).figures[stage].keys()
            figures[stage] = {f: sum(tr[typ].figures[stage][f] * n for typ, n in count.items()) for f in names}
    return Expect(rows, figures, entering)


def entering(layout, k, stages, stage):
    """(rows the stage is given, their marks, each group's first row among them), tiled."""
    layout = list(layout)
    rows, off = _tile(layout, lambda typ: trace(typ, k, stages).rows_in[stage])
    names = [n for n in trace(layout[0], k, stages).mark[stage] if n != "sizes"]
    marks = {n: _tile(layout, lambda typ: trace(typ, k, stages).mark[stage][n], qid=False)[0] for n in names}
    return rows, marks, off


# ------------------------------------------------------------- layouts ----

def cyclic(counts):
    """The groups of {type: how many} dealt out evenly: each type's groups at
    equal distances through the layout, so that no two blocks of one type
    follow each other where several types have many groups."""
    slots = []
    for j, (typ, n) in enumerate(counts.items()):
        slots += [((i + (j + 0.5) / len(counts)) / n, j, typ) for i in range(n)]
    return [typ for _, _, typ in sorted(slots)]


def rows_of(layout, k):
    n = {typ: len(group_rows(typ, k)) for typ in set(layout)}
    return [n[typ] for typ in layout]


def seam_inside(layout, k, straddler, filler):
    """`layout` with a group of type `straddler` put where its rows cross row
    CAP, after groups of the small type `filler` that bring the seam well
    inside it (for layouts whose rows are the search's: the pair cases)."""
    per = np.cumsum([0] + rows_of(layout, k))
    at = int(np.searchsorted(per, CAP, side="right")) - 1  # the group that holds row CAP
    gap = CAP - int(per[at])                                # rows from its first row to the seam
    n, f = len(group_rows(straddler, k)), len(group_rows(filler, k))
    fill = max(0, -(-(gap - n // 2) // f)) if gap >= n else 0
    return layout[:at] + [filler] * fill + [straddler] + layout[at:]


SMALL_PAIRS = {(1, 0, 0, 2): 8, (3, 0, 0, 5): 8, (7, 0, 0, 4): 8, (9, 0, 0, 10): 8, (63, 0, 0, 64): 8,
               (64, 0, 0, 65): 8, (65, 0, 0, 63): 8, (6, 0, 0, 0): 8, (0, 0, 0, 8): 8}
SMALL_SAME = {(c, 0, 0, c): 8 for c in (1, 2, 3, 5, 9, 63, 64, 65)}
SMALL_NONE = {(c, 0, 0, 0): 8 for c in (1, 2, 7, 10, 63, 64, 65)}
SMALL_NONE.update({(0, 0, 0, c): 8 for c in (3, 9, 64)})

BIG, ALL, NONE = (4097, 0, 0, 4096), (4097, 0, 0, 4097), (4097, 0, 0, 0)
# pairs, k = 0. The windows keep 1454, 4526 and 7962 of a BIG group's 8193 rows.
NARROW, MIDDLE, WIDE, SELF = (0, M + 30), (0, M + 100), (0, M + 400), (0, M)
PAIRS_PARTIAL = cyclic({BIG: 300, **SMALL_PAIRS})
PAIRS_ALL = cyclic({ALL: 280, **SMALL_SAME})           # with SELF: every row is its own partner's mate
PAIRS_NONE = cyclic({NONE: 560, **SMALL_NONE})
# every kind of group in one batch; a group without a kept row lies across the seam. SPARSE groups keep a
# few rows far apart: the first kept one comes after hundreds of dropped rows of its own pair (4097, 2049 first)
# or has the kept record before it, of its own pair, a thousand rows back or more (9 first)
SPARSE = {(4097, 0, 0, 64): 12, (2049, 0, 0, 9): 48, (9, 0, 0, 4097): 24}
PAIRS_MIXED = seam_inside(cyclic({BIG: 150, ALL: 70, NONE: 150, **SPARSE, **SMALL_PAIRS, **SMALL_SAME}), 0, NONE,
                          (63, 0, 0, 64))


def two_batches(layout, k):
    """(layout', batch): the groups of `layout` up to the one that takes the
    rows past CAP by more than 64 and the two after it, then as many small groups again, for a call
    with SAHARA_BATCH = batch patterns: batches are equal shares of the
    patterns (pass_plan.h batchStarts), so the first holds the big groups,
    slightly more than CAP rows, and the second the small ones."""
    per = np.cumsum(rows_of(layout, k))
    g = int(np.searchsorted(per, CAP + 64, side="right")) + 3
    small = list(SMALL_PAIRS) + list(SMALL_SAME)
    return layout[:g] + [small[i % len(small)] for i in range(g)], 4 * g


# loci, k = 1: u_2048 has 2048 exact copies and 7 with one substitution
TWINS = (2048, 0, 0, 2048)
SMALL_LOCI = {(3, 0, 0, 8): 8, (64, 0, 0, 9): 8, (8, 0, 0, 3): 8, (9, 0, 0, 64): 8, (65, 0, 0, 1): 8, (0, 0, 0, 63): 8}
LOCI = cyclic({TWINS: 550, **SMALL_LOCI})
LOCI_W = (22, 200, 100000)

# rescue, search k = 0: the partner's copies with one substitution are what the scans find
R64, R9 = (4097, 0, 0, 64), (2049, 0, 0, 9)
SMALL_RESCUE = {(65, 0, 0, 64): 6, (64, 0, 0, 9): 6, (63, 0, 0, 3): 6, (10, 0, 0, 8): 6, (9, 0, 0, 64): 6,
                (3, 0, 0, 2048): 6, (8, 0, 0, 3): 6}
RESCUE = cyclic({R64: 360, R9: 360, **SMALL_RESCUE})
RESCUE_WINDOW = (0, M + 4095)
RESCUE_CAP = 100  # above every small query's anchors, below the big ones'

# the chain, k = 0: loci at W = 22 leave more than CAP representatives, which the rescue scans,
# the pair rule cuts and --max_hits 3 cuts again
CHAIN = cyclic({BIG: 300, R64: 60, R9: 20, **SMALL_RESCUE, **SMALL_PAIRS})
CHAIN_STAGES = Stages(W=22, rescue=(3, 0), frag=(0, M + 1000), limit=3)
