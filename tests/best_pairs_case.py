"""The planted case of the best-pairs tests: two records and some two hundred
mate pairs made from their text, with the CPU oracle's all-mode rows. Every
shape that the rule (docs/semantics.md "Best pairs") distinguishes is planted
by name (`plan`): copies of a mate at different costs, ties, a dear mate shared
by two forward hits, both orientations of one pair, pairs without a mate,
mates inside long tandem runs. check() asserts each on the oracle's rows
through tests/best_pairs_model.py. No GPU: tests/test_best_pairs_gpu.py runs
it on one."""
import functools

import numpy as np

import oracle as O
import sahara_amd as sa
from best_pairs_model import NONE, best_pairs, scores
from helpers import acgt, hits_as_rows
from pairs_case import boundaries
from pairs_model import pairs
from test_golden import RC

SIGMA, M, K = 6, 48, 2
SEED = 11
# the fragment settings of the tests: a wide window, min == max, min == max == len
WIDE, EXACT, SAME = (100, 300), (200, 200), (M, M)
SETTINGS = (WIDE, EXACT, SAME)
DELTAS = (0, 1, 30)
RUN = 400  # symbols of a tandem run


def rc(x):
    return RC[SIGMA][np.asarray(x, np.uint8)][::-1]


def substitute(rng, x, n, lo=8, hi=M - 8):
    """n substitutions at distinct inner positions (with two of them nothing
    but the exact position lies within K = 2 edits)."""
    x = np.array(x, np.uint8)
    A = acgt(SIGMA)
    for j in rng.choice(np.arange(lo, hi), size=n, replace=False):
        x[j] = rng.choice(A[A != x[j]])
    return x


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(SEED)
    A = acgt(SIGMA)
    r0 = A[rng.integers(0, 4, size=40000)].astype(np.uint8)
    r1 = A[rng.integers(0, 4, size=3000)].astype(np.uint8)
    mates, plan = [], []

    def add(kind, a_mate, b_mate, **what):
        plan.append(dict(kind=kind, pair=len(mates), **what))
        mates.append((np.asarray(a_mate, np.uint8), np.asarray(b_mate, np.uint8)))

    def other(at):  # the text with one symbol changed: a copy that costs one substitution more
        r0[at] = rng.choice(A[A != r0[at]])

    # the text first: every copy is in place before a read is cut from it
    r0[2100:2148] = r0[2000:2048]   # "copy+1": mate B's place again 100 further ...
    other(2120)                     # ... one substitution dearer
    r0[3100:3148] = r0[3000:3048]   # "tie": the same, at the same cost
    r0[4180:4228] = r0[4000:4048]   # "shared": mate A's place again 180 further; mate B at 4100 ...
    r0[4240:4288] = r0[4100:4148]   # ... and, one substitution dearer, at 4240: the only mate of A at 4180
    other(4260)
    r0[7000:7200] = rc(r0[5000:5200])  # "orientations": the fragment at 5000 as its reverse complement at 7000 ...
    other(7170)                        # ... where rc A (at 7152) costs one substitution
    tandem = {}
    for unit, at in ((3, 20000), (5, 21000), (7, 22000)):
        r0[at:at + RUN] = np.resize(A[rng.integers(0, 4, size=unit)], RUN)
        other(at + 200)  # the run's one odd symbol: a read that covers it fits exactly at one place only
        tandem[at] = unit
    recs = [r0, r1]

    def proper(kind, a, F, edits, rec=0, **what):
        r = recs[rec]
        add(kind, substitute(rng, r[a:a + M], edits), substitute(rng, rc(r[a + F - M:a + F]), edits),
            seq=rec, a=a, b=a + F - M, F=F, **what)

    add("copy+1", r0[1900:1948], rc(r0[2000:2048]), seq=0, a=1900, b=2000, dear=2100)
    add("tie", r0[2900:2948], rc(r0[3000:3048]), seq=0, a=2900, b=3000, b2=3100)
    add("shared", r0[4000:4048], rc(r0[4100:4148]), seq=0, a=4000, a2=4180, b=4100, dear=4240)
    add("orientations", r0[5000:5048], rc(r0[5152:5200]), seq=0, a=5000, b=5152, fwd2=7000, rev2=7152)
    add("unmappable", r0[8000:8048], A[rng.integers(0, 4, size=M)], seq=0, a=8000)
    proper("lone", 8500, 200, 2)   # one placement and nothing near it within K: no next
    proper("clean", 9000, 200, 0)  # one placement at no cost, its neighbours at pos +- 1 cost 1 each
    for at, unit in tandem.items():
        # mate A left of the run, mate B inside it over the odd symbol: its exact place and, a unit
        # apart, hundreds of dearer ones in the window
        add("tandem", r0[at - 50:at - 2], rc(r0[at + 180:at + 228]), seq=0, a=at - 50, b=at + 180, unit=unit)
        # both mates inside the run, away from the odd symbol: every shift ties
        add("tandem tie", r0[at + 250:at + 298], rc(r0[at + 330:at + 378]), seq=0, unit=unit)
    for i in range(150):  # the bulk: proper pairs all over both records
        rec = 1 if i % 8 == 0 else 0
        F = EXACT[0] if i % 3 == 0 else M if i % 10 == 1 else int(rng.integers(60, 360))
        a = int(rng.integers(0, len(recs[rec]) - F))
        proper("bulk", a, F, i % 3, rec)
    order = rng.permutation(len(mates))
    where = np.argsort(order)  # pair `p` of the plan is pair where[p] of the reads
    for e in plan:
        e["pair"] = int(where[e["pair"]])
    reads = np.ascontiguousarray(np.stack([m for i in order for m in mates[i]]).astype(np.uint8))
    pats = sa.interleave_rc(reads, SIGMA)
    scheme = sa.search_scheme("h2-k2", 0, K, M)
    ref = O.Index.build(recs, SIGMA, 16)
    want = hits_as_rows(ref.search(pats, scheme, edit=True, nthreads=8)[0])
    return dict(sigma=SIGMA, recs=recs, reads=reads, pats=pats, scheme=scheme, ref=ref, want=want, plan=plan,
                n_pairs=len(reads) // 2)


@functools.lru_cache(maxsize=None)
def expected(setting, delta, rows_key="want"):
    """(kept rows, summary) of the model on the oracle's rows."""
    c = planted()
    return best_pairs(c[rows_key], M, *setting, delta, c["n_pairs"])


@functools.lru_cache(maxsize=None)
def check():
    """What the GPU tests rely on, asserted on the oracle's rows."""
    c = planted()
    w = c["want"]
    assert len(c["reads"]) % 2 == 0 and len(c["reads"]) <= 1000
    assert len(w) <= 2_000_000
    paired = {s: set(map(tuple, pairs(w, M, *s)[:, :3].tolist())) for s in SETTINGS}
    n_paired = {s: len(pairs(w, M, *s)) for s in SETTINGS}
    kept = {(s, d): set(map(tuple, expected(s, d)[0][:, :3].tolist())) for s in SETTINGS for d in DELTAS}
    summ = {(s, d): expected(s, d)[1] for s in SETTINGS for d in DELTAS}
    by = {}
    for e in c["plan"]:
        by.setdefault(e["kind"], []).append(e)

    def one(kind):
        assert len(by[kind]) == 1, kind
        return by[kind][0]

    def has_mate(s, key):
        return key in paired[s]

    # a dearer copy of mate B in the window: dropped at delta 0, back at delta 1
    e = one("copy+1")
    A, B, D = (4 * e["pair"], 0, e["a"]), (4 * e["pair"] + 3, 0, e["b"]), (4 * e["pair"] + 3, 0, e["dear"])
    assert has_mate(WIDE, D)
    assert A in kept[WIDE, 0] and B in kept[WIDE, 0] and D not in kept[WIDE, 0] and D in kept[WIDE, 1]
    assert summ[WIDE, 0][e["pair"]]["best"] == 0 and summ[WIDE, 0][e["pair"]]["next"] == 1
    assert tuple(summ[WIDE, 0][e["pair"]][["n_fwd", "n_rev"]]) == (1, 1)
    # an exact tie: both kept
    e = one("tie")
    B, B2 = (4 * e["pair"] + 3, 0, e["b"]), (4 * e["pair"] + 3, 0, e["b2"])
    assert B in kept[WIDE, 0] and B2 in kept[WIDE, 0]
    assert tuple(summ[WIDE, 0][e["pair"]][["best", "n_fwd", "n_rev"]]) == (0, 1, 2)
    # a forward hit with a cheap and a dear mate; the dear one is the only mate of another forward hit
    e = one("shared")
    A, A2 = (4 * e["pair"], 0, e["a"]), (4 * e["pair"], 0, e["a2"])
    B, D = (4 * e["pair"] + 3, 0, e["b"]), (4 * e["pair"] + 3, 0, e["dear"])
    assert all(has_mate(WIDE, x) for x in (A, A2, B, D))
    assert A in kept[WIDE, 0] and B in kept[WIDE, 0] and A2 not in kept[WIDE, 0] and D not in kept[WIDE, 0]
    assert A2 in kept[WIDE, 1] and D in kept[WIDE, 1]
    # both orientations concordant: the dearer one goes at delta 0
    e = one("orientations")
    A, B = (4 * e["pair"], 0, e["a"]), (4 * e["pair"] + 3, 0, e["b"])
    F2, R2 = (4 * e["pair"] + 2, 0, e["fwd2"]), (4 * e["pair"] + 1, 0, e["rev2"])
    for s in (WIDE, EXACT):
        assert has_mate(s, F2) and has_mate(s, R2)
        assert A in kept[s, 0] and B in kept[s, 0] and F2 not in kept[s, 0] and R2 not in kept[s, 0]
        assert F2 in kept[s, 1] and R2 in kept[s, 1]
    # no mate anywhere
    e = one("unmappable")
    assert any(r[0] // 4 == e["pair"] for r in map(tuple, w[:, :3].tolist()))
    for key in summ:
        assert tuple(summ[key][e["pair"]]) == (NONE, NONE, 0, 0, 0), key
    # next: none, and best + 2 (min == max: a neighbour's mate is a neighbour too, one error each)
    e = one("lone")
    for s in (WIDE, EXACT):
        assert tuple(summ[s, 0][e["pair"]]) == (4, NONE, 1, 1, 0), s
    e = one("clean")
    assert tuple(summ[EXACT, 0][e["pair"]]) == (0, 2, 1, 1, 0)
    assert summ[WIDE, 0][e["pair"]]["next"] == 1
    # tandem runs: the exact copy beats the shifted ones, of which a window holds hundreds
    size = np.zeros(len(w), np.int64)
    scores(w, M, *WIDE, counts=size)
    for e in by["tandem"]:
        B = (4 * e["pair"] + 3, 0, e["b"])
        shifted = (4 * e["pair"] + 3, 0, e["b"] - e["unit"])
        assert has_mate(WIDE, shifted) and B in kept[WIDE, 0] and shifted not in kept[WIDE, 0], e
        assert tuple(summ[WIDE, 0][e["pair"]][["best", "n_fwd", "n_rev"]]) == (0, 1, 1), e
    for e in by["tandem tie"]:
        assert summ[WIDE, 0][e["pair"]]["n_rev"] >= 20 and summ[WIDE, 0][e["pair"]]["n_fwd"] >= 20, e
    assert size.max() > 256 + 64, size.max()  # a range across several 64-record blocks and a 256-thread workgroup
    assert (size > 256).sum() >= 100
    # duplicates of one position with different err: exactly one is kept (the first)
    full = expected(WIDE, 30)[0]
    assert len(np.unique(full[:, :3], axis=0)) == len(full)
    rows_p = pairs(w, M, *WIDE)
    dup = (rows_p[1:, :3] == rows_p[:-1, :3]).all(axis=1) & (rows_p[1:, 3] != rows_p[:-1, 3])
    assert dup.sum() >= 10, dup.sum()
    # a pair whose qids an ungrained SAHARA_BATCH=7 cut would split, with kept hits on both sides
    cut = [b for b in boundaries(len(c["pats"]), 7) if b % 4]
    assert any({r[0] for r in kept[WIDE, 0] if r[0] // 4 == b // 4 and r[0] < b} and
               {r[0] for r in kept[WIDE, 0] if r[0] // 4 == b // 4 and r[0] >= b} for b in cut)
    for s in SETTINGS:
        sizes = [len(expected(s, d)[0]) for d in DELTAS]
        assert len(set(sizes)) == 3 and all(0 < n < n_paired[s] for n in sizes), (s, sizes)
    return c
