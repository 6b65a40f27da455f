"""A text whose hit counts are known by construction (CPU only, numpy only).

Every count c of COUNTS has one random A C G T unit u_c of M symbols, planted
c times exactly and, for the counts of SUBS, SUBS[c] more times with one
substitution each. All copies stand in one seeded random order, each followed
by 1 to 3 random symbols, and the sequence is cut into records at copy
boundaries. A query that is u_c therefore finds, under Hamming distance with
bound k, every planted copy of u_c with at most k substitutions, at that e,
and nothing else; a random pattern finds nothing. tests/test_planted_model.py
proves this equal to the oracle's rows for the committed seeds, which is what
lets tests/test_hit_chain_edges.py take the construction as its expectation:
rows of a million queries without an oracle run, already in canonical
(qid, seq_id, pos, err) order.

The query layouts of test_hit_chain_edges.py are data here (lists of counts;
0 = a random pattern), so that the properties they exist for are asserted
without a GPU. A "range" is 256 consecutive queries from the start of a batch:
one workgroup of the sort (locate_sort.hip kSortDecode).
"""
import functools

import numpy as np

from helpers import acgt

M = 20
SEED = 20261020
COUNTS = tuple(range(1, 11)) + (63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
# count -> copies with one substitution; (3, 5), (8, 1), (64, 5), (2048, 7) are the --max_hits pairs
SUBS = {3: 5, 8: 1, 9: 3, 64: 5, 2048: 7}
LIMIT_PAIRS = ((3, 5), (8, 1), (64, 5), (2048, 7))
N_RANDOM = 16  # patterns for count 0

# the sort's tiers (locate_sort.hip): rows <= SMALL in a lane, <= MEDIUM in a wave,
# <= LDS in a workgroup's LDS, more by the segmented radix sort; a range of
# <= TILE rows is staged in LDS; the scan works on tiles of SCAN_TILE counts
SMALL, MEDIUM, LDS, TILE, RANGE, SCAN_TILE = 8, 64, 2048, 1024, 256, 4096
LONG_COUNTS = (65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


def tier(n):
    return ("zero" if n == 0 else "small" if n <= SMALL else "medium" if n <= MEDIUM else
            "long" if n <= LDS else "huge")


class Planted:
    """records: list of uint8 rank arrays; unit[c]: u_c; table[c]: (copies, 3)
    int64 array of (record, position, substitutions) in (record, position)
    order; random: (N_RANDOM, M) patterns that occur nowhere."""

    def __init__(self, records, unit, table, random, sigma):
        self.records, self.unit, self.table, self.random, self.sigma = records, unit, table, random, sigma
        self.n_symbols = int(sum(len(r) for r in records))

    def patterns(self, layout):
        """(len(layout), M) uint8: query i is u_{layout[i]}, or a random pattern for 0."""
        layout = np.asarray(layout, np.int64)
        vals, inv = np.unique(layout, return_inverse=True)
        tab = np.stack([self.unit[int(c)] if c else self.random[0] for c in vals])
        pats = tab[inv]
        zero = np.flatnonzero(layout == 0)
        pats[zero] = self.random[zero % N_RANDOM]
        return np.ascontiguousarray(pats)

    def block(self, c, k):
        """(rows, 3) uint64 (seq_id, pos, err) of one query u_c under Hamming k, canonical order."""
        if c == 0:
            return np.zeros((0, 3), np.uint64)
        t = self.table[int(c)]
        return t[t[:, 2] <= k].astype(np.uint64)

    def expected(self, layout, k=0, qid0=0):
        """Canonical (qid, seq_id, pos, err) rows of the query list, qids from qid0."""
        layout = np.asarray(layout, np.int64)
        vals = np.unique(layout)
        blocks = {int(c): self.block(c, k) for c in vals}
        per_q = np.zeros(len(layout), np.int64)
        for c, b in blocks.items():
            per_q[layout == c] = len(b)
        off = np.concatenate([[0], np.cumsum(per_q)])
        out = np.empty((int(off[-1]), 4), np.uint64)
        for c, b in blocks.items():
            if len(b) == 0:
                continue
            q = np.flatnonzero(layout == c)
            dst = (off[q][:, None] + np.arange(len(b))[None, :]).ravel()
            out[dst, 1:] = np.tile(b, (len(q), 1))
            out[dst, 0] = np.repeat(q + qid0, len(b)).astype(np.uint64)
        return out

    def per_query(self, layout, k=0):
        """Rows per query of the layout under Hamming k."""
        n = {int(c): len(self.block(c, k)) for c in np.unique(layout)}
        return np.array([n[int(c)] for c in layout], np.int64)


@functools.lru_cache(maxsize=None)
def build(sigma=6, nrec=5):
    """The planted text in `nrec` records. The same seeded symbol sequence for
    every nrec and sigma (dna4: T is rank 4, not 5); only the cuts differ."""
    rng = np.random.default_rng(SEED)
    alpha = acgt(sigma)
    unit = {c: rng.integers(0, 4, M) for c in COUNTS}
    random = rng.integers(0, 4, (N_RANDOM, M))
    items = [(c, 0) for c in COUNTS for _ in range(c)] + [(c, 1) for c, s in SUBS.items() for _ in range(s)]
    items = [items[i] for i in rng.permutation(len(items))]
    per_rec = [[] for _ in range(nrec)]
    rows = {c: [] for c in COUNTS}
    pos = [0] * nrec
    for j, (c, s) in enumerate(items):
        r = j * nrec // len(items)
        u = unit[c].copy()
        if s:
            p = rng.integers(0, M)
            u[p] = (u[p] + rng.integers(1, 4)) % 4
        spacer = rng.integers(0, 4, rng.integers(1, 4))
        rows[c].append((r, pos[r], s))
        per_rec[r] += [u, spacer]
        pos[r] += M + len(spacer)
    records = [alpha[np.concatenate(p)].astype(np.uint8) for p in per_rec]
    table = {}
    for c, t in rows.items():
        t = np.array(sorted(t), np.int64).reshape(-1, 3)
        t.setflags(write=False)
        table[c] = t
    for r in records:
        r.setflags(write=False)
    return Planted(records, {c: alpha[u].astype(np.uint8) for c, u in unit.items()}, table,
                   alpha[random].astype(np.uint8), sigma)


# ------------------------------------------------------------ layouts ----

def _range(head, fill):
    """One range: `head`, then `fill` repeated to RANGE queries."""
    out = list(head)
    i = 0
    while len(out) < RANGE:
        out.append(fill[i % len(fill)])
        i += 1
    assert len(out) == RANGE
    return out


def _fill_to(head, total):
    """One range of `head` and fillers of 3 and 4 rows that sums to `total` rows."""
    rest, n = total - sum(head), RANGE - len(head)
    fours = rest - 3 * n
    assert 0 <= fours <= n
    body = [4 if (i * fours) // n != ((i + 1) * fours) // n else 3 for i in range(n)]
    return list(head) + body


EDGE_HEAD = [0, 1, 8, 9, 64, 65, 63, 10]
# (a) named ranges; every tier edge in one range of exactly TILE rows, and its twin of TILE + 1
RANGES_A = {
    "edges_1024": _fill_to(EDGE_HEAD, TILE),
    "edges_1025": _fill_to(EDGE_HEAD, TILE + 1),
    "256x4": [4] * RANGE,
    "1024_alone": _range([1024], [0]),
    "16x64": _range([64] * 16, [0]),
    # wave 1 (queries 64..127) holds 64 medium queries: the ballot loop runs 64 times
    "wave_medium": _range([1] * 64 + [9, 10] * 32, [0]),
    "wave_medium_global": _range([1] * 64 + [9, 10] * 32 + [1023], [0]),
    "full_before": [4] * RANGE,
    "zeros": [0] * RANGE,
    "full_after": [4] * RANGE,
}
LAYOUT_A = [c for r in RANGES_A.values() for c in r]


def _place(n, fill, at):
    out = [fill[i % len(fill)] for i in range(n)]
    for i, c in at.items():
        out[i % n] = c
    return out


_SMALLS = (1, 0, 3, 9, 2, 0, 1, 4)
# (b) every long and huge edge; a long and a huge query first in the batch,
# last in it (the end is the sentinel) and on both sides of a range boundary
LAYOUT_B1 = _place(300, _SMALLS, {0: 65, **{10 + 7 * i: c for i, c in enumerate(LONG_COUNTS)},
                                   255: 2049, 256: 65, 299: 2049})
LAYOUT_B2 = _place(300, _SMALLS, {0: 2049, **{11 + 5 * i: c for i, c in enumerate(LONG_COUNTS)},
                                   255: 2048, 256: 4097, 299: 65})

# (c) query counts around a range and around a scan tile
NQ_EDGES = (1, 255, 256, 257, 4095, 4096, 4097)


def layout_c(nq):
    """nq queries; the last one long (its end is the sentinel), the one before it huge."""
    at = {nq - 1: 65}
    if nq > 2:
        at[nq - 2] = 2049
    return _place(nq, _SMALLS, at)


# (d) more patterns than kScanPartials scans in one trip (256 tiles of SCAN_TILE)
ONE_TRIP = 256 * SCAN_TILE
NQ_D = ONE_TRIP + 300
_CYCLE_D = (0, 1, 2, 3, 1, 0, 1, 4)


def layout_d():
    lay = np.resize(np.array(_CYCLE_D, np.int64), NQ_D)
    lay[ONE_TRIP + 100] = 65    # listed from a tile whose offset is the carried sum
    lay[ONE_TRIP + 200] = 2049
    return lay


# (e) grid caps
BIG_LDS_GRID = 4096            # kSortBigLds' workgroups; also llist's entries (SCAN_TILE)
LAYOUT_E_65 = [65] * 4200
# 2048s in both scan tiles: a workgroup's second (strided) trip meets 2048 rows after 65 and 65 after 2048
LAYOUT_E_MIXED = _place(4200, (65,), {**{i * 40 + 7: 2048 for i in range(100)}, 4100: 2048, 4103: 65, 4150: 2048,
                                      4199: 2048})
LAYOUT_E_LLIST = [65] * SCAN_TILE + [1, 0, 65, 3]
LAYOUT_E_2M = [4097] * 600     # > 8192 * 256 hits
LAYOUT_E_4M = [4097] * 1100    # > 16384 * 256 hits
# kOffsetSeq runs once per part over that part's hits: enough queries that one
# part of the three-part index alone passes 8192 * 256 (hits_per_part)
LAYOUT_E_PARTS = [4097] * 1300
PART_SYMBOLS = 200000          # SAHARA_PART_SYMBOLS that builds the 5-record text as three parts
CAP_8192 = 8192 * 256
CAP_16384 = 16384 * 256

def split_records(records, limit=PART_SYMBOLS):
    """First record of each part, and the record count last (index_build.hip
    splitRecords: records fill a part while their symbols, one delimiter each
    included, stay within `limit`)."""
    first, n = [0], 0
    for r, rec in enumerate(records):
        if n and n + len(rec) + 1 > limit:
            first.append(r)
            n = 0
        n += len(rec) + 1
    return first + [len(records)]


def hits_per_part(t, layout, k=0, limit=PART_SYMBOLS):
    """Rows of the layout's queries in each part of the text's multi-part index."""
    first = np.array(split_records(t.records, limit))
    out = np.zeros(len(first) - 1, np.int64)
    for c, n in zip(*np.unique(np.asarray(layout), return_counts=True)):
        rec = t.block(int(c), k)[:, 0].astype(np.int64)
        out += n * np.bincount(np.searchsorted(first, rec, side="right") - 1, minlength=len(out))
    return out


# (g) part merge: pattern counts around sortHitsByQid's endBit steps
NQ_PARTS = (1, 2, 3, 4, 5, 1024, 1025)


def layout_g(nq):
    return [LONG_COUNTS[i % len(LONG_COUNTS)] for i in range(nq)]


# section 4: --max_hits n at the quota edges of (c0 exact, c1 one-substitution) copies
def limit_cases():
    """[(c0, c1, n, branch)]: branch is what limitPlan does with the query u_c0 at Hamming k = 1."""
    out = []
    for c0, c1 in LIMIT_PAIRS:
        for n in sorted({c0 - 1, c0, c0 + 1, c0 + c1 - 1, c0 + c1, c0 + c1 + 1}):
            if n < 1:
                continue
            if c0 + c1 <= n:
                branch = "all kept"           # distinct <= n
            elif n <= c0:
                branch = "ends at level 0" if n == c0 else "cut inside level 0"
            else:
                branch = "cut inside level 1"  # cum = c0 < n < c0 + c1
            out.append((c0, c1, n, branch))
    return out
