"""The planted case of the pair tests: two records and a few hundred mate
pairs made from their text (mate A from [a, a + len) with 0-2 substitutions,
mate B the reverse complement of [a + F - len, a + F)), with the CPU oracle's
all-mode rows. Every shape the rule distinguishes is planted by name
(`plan`), and check() asserts each on the oracle's rows through
tests/pairs_model.py. No GPU: tests/test_pairs_gpu.py runs it on one."""
import functools

import numpy as np

import oracle as O
import sahara_amd as sa
from helpers import acgt, hits_as_rows
from pairs_model import pair_count, pairs
from test_golden import RC

SIGMA, M, K = 6, 48, 2
SEED = 5
# the fragment settings of the tests: a wide window, min == max, min == max == len
WIDE, EXACT, SAME = (100, 300), (200, 200), (M, M)
SETTINGS = (WIDE, EXACT, SAME)


def rc(x):
    return RC[SIGMA][np.asarray(x, np.uint8)][::-1]


def substitute(rng, x, n, lo=8, hi=M - 8):
    """n substitutions at distinct inner positions: with two of them nothing
    but the exact position lies within K = 2 edits, so the pair's distance is
    exactly what was planted."""
    x = np.array(x, np.uint8)
    A = acgt(SIGMA)
    for j in rng.choice(np.arange(lo, hi), size=n, replace=False):
        x[j] = rng.choice(A[A != x[j]])
    return x


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(SEED)
    A = acgt(SIGMA)
    r0 = A[rng.integers(0, 4, size=30000)]
    r1 = A[rng.integers(0, 4, size=3000)]
    seg = A[rng.integers(0, 4, size=120)]
    for at in (5000, 5180, 9000, 15000):  # two copies 180 apart, two far away
        r0[at:at + 120] = seg
    r1[1000:1120] = seg
    tandem = {}
    for unit, at in ((3, 20000), (5, 21000), (7, 22000)):
        r0[at:at + 160] = np.resize(A[rng.integers(0, 4, size=unit)], 160)
        tandem[at] = unit
    recs = [r0.astype(np.uint8), r1.astype(np.uint8)]
    mates, plan = [], []

    def add(kind, a_mate, b_mate, **what):
        plan.append(dict(kind=kind, pair=len(mates), **what))
        mates.append((np.asarray(a_mate, np.uint8), np.asarray(b_mate, np.uint8)))

    def proper(kind, a, F, edits, rec=0, **what):
        r = recs[rec]
        add(kind, substitute(rng, r[a:a + M], edits), substitute(rng, rc(r[a + F - M:a + F]), edits),
            seq=rec, a=a, b=a + F - M, F=F, **what)

    free = iter(range(400, 4400, 400))  # unique text, away from everything planted
    for F, kind in ((WIDE[0], "F=min"), (WIDE[0] - 1, "F=min-1"), (WIDE[1], "F=max"), (WIDE[1] + 1, "F=max+1"),
                    (EXACT[0], "F=200"), (EXACT[0] + 1, "F=201"), (M, "F=len"), (M + 1, "F=len+1")):
        proper(kind, next(free), F, 2)
    proper("near 0", 0, 58, 2)  # the reverse mate at pos 10, below the wide setting's dmin = 52
    a = 26000
    add("other record", substitute(rng, r0[a:a + M], 1), substitute(rng, rc(r1[500:500 + M]), 1), seq=0, a=a)
    add("reverse/forward", substitute(rng, r0[a + 500:a + 500 + M], 1), substitute(rng, rc(r0[a + 350:a + 350 + M]), 1),
        seq=0, a=a + 500)
    add("both forward", substitute(rng, r0[a + 1000:a + 1000 + M], 1), substitute(rng, r0[a + 1150:a + 1150 + M], 1),
        seq=0, a=a + 1000)
    add("unmappable", substitute(rng, r0[a + 1500:a + 1500 + M], 1), A[rng.integers(0, 4, size=M)], seq=0, a=a + 1500)
    # mate B inside the segment: one copy in the wide window, one 180 further, two far away, one in r1
    for i in range(12):
        a, off = 4860 + 7 * i, 5 * i
        add("copies", substitute(rng, r0[a:a + M], i % 3), substitute(rng, rc(seg[off:off + M]), i % 3), seq=0, a=a,
            b=5000 + off)
    # ... and mate A inside it, mate B in unique text right of the first copy
    for i in range(4):
        off, b = 10 * i, 5330 + 9 * i
        add("copies A", substitute(rng, seg[off:off + M], i % 3), substitute(rng, rc(r0[b:b + M]), i % 3), seq=0,
            a=5000 + off, b=b)
    # a mate inside a tandem run: hundreds of rows, some in the window and some not
    for at, unit in tandem.items():
        run = r0[at:at + 160]
        add("tandem B", substitute(rng, r0[at - 130:at - 130 + M], 1), substitute(rng, rc(run[40:40 + M]), 1, 20, 28),
            seq=0, a=at - 130)
        add("tandem A", substitute(rng, run[60:60 + M], 1, 20, 28), substitute(rng, rc(r0[at + 250:at + 250 + M]), 1),
            seq=0, b=at + 250)
        add("tandem both", run[30:30 + M], rc(run[30:30 + M]), seq=0)  # F == len inside the run
    # the bulk: proper pairs all over both records, a third at F == 200 and a tenth at F == len
    for i in range(200):
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
    return dict(sigma=SIGMA, recs=recs, reads=reads, pats=pats, scheme=scheme, ref=ref, want=want, plan=plan)


@functools.lru_cache(maxsize=None)
def kept(setting, rows_key="want"):
    return pairs(planted()[rows_key], M, *setting)


def boundaries(npat, batch):
    """The batch boundaries of npat patterns in equal batches of at most
    `batch` (pass_plan.h batchStarts without a granularity)."""
    n = -(-npat // batch)
    return [npat * i // n for i in range(n + 1)]


@functools.lru_cache(maxsize=None)
def check():
    """What the GPU tests rely on, asserted on the oracle's rows."""
    c = planted()
    w = c["want"]
    assert len(c["reads"]) % 2 == 0 and 400 <= len(c["reads"]) <= 1000
    assert len(w) <= 2_000_000
    rows = {s: set(map(tuple, kept(s)[:, :3].tolist())) for s in SETTINGS}
    every = set(map(tuple, w[:, :3].tolist()))
    by = {}
    for e in c["plan"]:
        by.setdefault(e["kind"], []).append(e)

    def fwd(e):  # the planted placement of mate A: (qid, seq_id, pos)
        return (4 * e["pair"], e["seq"], e["a"])

    def rev(e):  # ... of the reverse complement of mate B
        return (4 * e["pair"] + 3, e["seq"], e["b"])

    def one(kind):
        assert len(by[kind]) == 1, kind
        return by[kind][0]

    for kind, setting, inside in (("F=min", WIDE, True), ("F=min-1", WIDE, False), ("F=max", WIDE, True),
                                  ("F=max+1", WIDE, False), ("F=200", EXACT, True), ("F=201", EXACT, False),
                                  ("F=len", SAME, True), ("F=len+1", SAME, False)):
        e = one(kind)
        assert fwd(e) in every and rev(e) in every, kind
        assert (fwd(e) in rows[setting]) == inside and (rev(e) in rows[setting]) == inside, kind
    e = one("F=len")
    assert e["a"] == e["b"]  # both mates at one position
    e = one("near 0")
    dmin = WIDE[0] - M
    assert rev(e) in every and e["b"] < dmin and rev(e) not in rows[WIDE]
    assert any(q % 2 == 1 and p < dmin for q, _, p in every)
    for kind in ("other record", "reverse/forward", "both forward", "unmappable"):
        e = one(kind)
        mine = [r for r in every if r[0] // 4 == e["pair"]]
        assert fwd(e) in mine, kind
        assert not any(r[0] // 4 == e["pair"] for s in SETTINGS for r in rows[s]), kind
        qids = {r[0] % 4 for r in mine}
        seqs = {r[0] % 4: r[1] for r in mine}
        if kind == "other record":
            assert {0, 3} <= qids and seqs[0] != seqs[3]
        if kind == "reverse/forward":
            assert {0, 3} <= qids and min(r[2] for r in mine if r[0] % 4 == 3) < e["a"] - M
        if kind == "both forward":
            assert {0, 2} <= qids and not {1, 3} & qids
        if kind == "unmappable":
            assert qids <= {0, 1}
    # queries that keep some hits and lose others
    some = 0
    for q in np.unique(w[:, 0]).tolist():
        n_all = sum(1 for r in every if r[0] == q)
        n_kept = sum(1 for r in rows[WIDE] if r[0] == q)
        some += 0 < n_kept < n_all
    assert some >= 10, some
    # partner segments of 256 records and more
    counts = dict(zip(*[x.tolist() for x in np.unique(w[:, 0], return_counts=True)]))
    big = sum(1 for q in counts if counts.get(q ^ 3, 0) >= 256)
    assert big >= 5, big
    assert max(counts.values()) <= 20000, max(counts.values())  # (test_pairs_model.py restates the rule in O(n^2) per pair)
    # a pair whose qids an ungrained SAHARA_BATCH=7 cut would split, with kept hits on both sides
    cut = [b for b in boundaries(len(c["pats"]), 7) if b % 4]
    assert any({r[0] for r in rows[WIDE] if r[0] // 4 == b // 4 and r[0] < b} and
               {r[0] for r in rows[WIDE] if r[0] // 4 == b // 4 and r[0] >= b} for b in cut)
    sizes = [len(kept(s)) for s in SETTINGS]
    assert len(set(sizes)) == 3 and all(0 < n < len(w) for n in sizes), sizes
    assert len({pair_count(kept(s)) for s in SETTINGS}) == 3
    return c
