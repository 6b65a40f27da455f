"""The planted case of the mate-rescue tests: two records and some eighty mate
pairs made from their text, one mate within the search's K = 2 substitutions
and the other carrying 3 to 12 edits, so that the search finds the first
alone and the rescue has to find the second in the fragment window. Every
shape the rule distinguishes is planted by name (`plan`), and check() asserts
each on the model (tests/rescue_model.py) over the CPU oracle's all-mode rows.
No GPU: tests/test_rescue_gpu.py runs it on one."""
import functools

import numpy as np

import oracle as O
import sahara_amd as sa
from helpers import acgt, hits_as_rows
from pairs_case import K, M, SIGMA, rc, substitute
from pairs_model import pairs
from rescue_model import anchors, rescue, scan

SEED = 11
KS = (3, 5, 8)
# the fragment settings: windows of 253 starts (the tests' main one), 1, 63, 64, 65 and 129 starts: a wave's
# round boundaries; dmin = 52 in all but the second
MAIN, ONE = (100, 352), (200, 200)
W63, W64, W65, W129 = (100, 162), (100, 163), (100, 164), (100, 228)
SETTINGS = (MAIN, ONE, W63, W64, W65, W129)
DMIN, DMAX = MAIN[0] - M, MAIN[1] - M
CAP = 8  # the tests' anchor cap: the tandem query has more


def mutate(rng, r, b, subs, ins=0, dele=0, n_at=None):
    """A pattern of M symbols that fits r at b with subs + ins + dele edits:
    `dele` text symbols dropped (a D each), `ins` symbols put in (an I each),
    `subs` symbols changed, all at distinct inner places at least 4 apart (3
    where there are more than 9); n_at: the place of one of the
    substitutions, which becomes an N."""
    A = acgt(SIGMA)
    t = list(np.asarray(r[b:b + M + dele - ins], np.uint8))
    step = 4 if subs + ins + dele <= (M - 10) // 4 else 3
    places = 5 + step * rng.permutation((M - 10) // step)[:subs + ins + dele]
    kinds = ["X"] * subs + ["I"] * ins + ["D"] * dele
    if n_at is not None:
        places[0] = n_at
    for at, kind in sorted(zip(places.tolist(), kinds), reverse=True):  # from the right: places stay put
        if kind == "D":
            del t[at]
        elif kind == "I":
            t.insert(at, int(rng.choice(A[(A != t[at]) & (A != t[at - 1])])))
        else:
            t[at] = 4 if at == n_at else int(rng.choice(A[A != t[at]]))
    assert len(t) == M
    return np.array(t, np.uint8)


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(SEED)
    A = acgt(SIGMA)
    r0 = A[rng.integers(0, 4, size=30000)].astype(np.uint8)
    r1 = A[rng.integers(0, 4, size=3000)].astype(np.uint8)
    recs = [r0, r1]
    mates, plan = [], []

    def add(kind, a_mate, b_mate, **what):
        plan.append(dict(kind=kind, pair=len(mates), **what))
        mates.append((np.asarray(a_mate, np.uint8), np.asarray(b_mate, np.uint8)))

    # The anchor is mate A at a (two substitutions: its only hit), the missing mate is rc B, whose text lies
    # at b = a + d with `edits`; e: what the rescue reports there (None: nothing within any K)
    def right(kind, a, d, edits, rec=0, e="sum", a_subs=2, n_at=None, **what):
        r = recs[rec]
        b = a + d
        bt = mutate(rng, r, b, *edits, n_at=n_at) if not isinstance(edits, np.ndarray) else edits
        add(kind, substitute(rng, r[a:a + M], a_subs), rc(bt), seq=rec, anchor=(0, a), found=(3, b),
            e=sum(edits) if e == "sum" else e, d=d, **what)

    # The anchor is rc B at b (an odd qid: the window lies to its left), the missing mate is A at a = b - d
    def left(kind, b, d, edits, rec=0, e="sum", **what):
        r = recs[rec]
        a = b - d
        add(kind, mutate(rng, r, a, *edits), rc(substitute(rng, r[b:b + M], 2)), seq=rec, anchor=(3, b), found=(0, a),
            e=sum(edits) if e == "sum" else e, d=d, **what)

    free = iter(range(400, 19600, 400))  # unique text, away from everything that changes the text below
    for edits in ((3,), (4,), (5,), (8,), (2, 1, 0), (2, 1, 1), (3, 1, 1), (6, 1, 1), (2, 0, 1)):
        right("errors", next(free), 150, edits)
    for n in (9, 12):
        right("too many", next(free), 150, (n,), e=None)
    # the best start at the window's edges, and one start outside: with 8 edits a shifted placement costs 9 or more
    for subs in (3, 8):
        right("at lo", next(free), DMIN, (subs,))
        right("at hi", next(free), DMAX, (subs,))
        right("below lo", next(free), DMIN - 1, (subs,), e=None, shifted=subs == 3)
        right("above hi", next(free), DMAX + 1, (subs,), e=None, shifted=subs == 3)
    # index 62, 63, 64, 100 (the 1-start window's) and 128 of the window: the last starts of the narrow
    # settings, and the first lanes of a wave's second and third round
    for d in (DMIN + 62, DMIN + 63, DMIN + 64, ONE[0] - M, DMIN + 128):
        right("round edge", next(free), d, (3,))
    # windows clipped by the record's end (r0's is followed by r1, r1's by the text's end) and by position 0
    right("clipped at end", len(r0) - M - 100, 100, (3,))
    right("clipped at end", len(r1) - M - 60, 60, (4,), rec=1)
    left("clipped at 0", 120, 120, (3,))
    left("clipped at 0", 90, 88, (3,), rec=1)
    # a mate that would lie across r0's '$': its last 28 symbols are r1's first
    a = len(r0) - M - 80
    right("across $", a, len(r0) - 20 - a, np.concatenate([r0[-20:], r1[:28]]), e=None)
    # copies of the mate's text inside one window (the text changes: r0[20000:26000] is theirs)
    def copies(kind, at, d1, d2, extra1, extra2, win):
        seg = r0[at + d1:at + d1 + M].copy()
        for d, extra in ((d1, extra1), (d2, extra2)):
            r0[at + d:at + d + M] = seg
            for j in (3, M - 5)[:extra]:  # (outside the places substitute() changes)
                r0[at + d + j] = A[(np.flatnonzero(A == seg[j])[0] + 1) % 4]
        bt = substitute(rng, seg, 3)
        add(kind, substitute(rng, r0[at:at + M], 2), rc(bt), seq=0, anchor=(0, at), found=(3, at + (d1, d2)[win]),
            e=3 + (extra1, extra2)[win], other=(at + (d2, d1)[win], 3 + (extra2, extra1)[win]), d=(d1, d2)[win])
    copies("tie in a round", 20000, DMIN + 5, DMIN + 58, 0, 0, 0)
    copies("tie across rounds", 20500, DMIN + 48, DMIN + 148, 0, 0, 0)
    copies("cheaper later", 21000, DMIN + 8, DMIN + 148, 2, 0, 1)
    copies("dearer later", 21500, DMIN + 8, DMIN + 148, 0, 2, 0)
    # an anchor with duplicates at its position and neighbours at p +- 1, p +- 2: mate A as the text has it
    for a_subs in (0, 1):
        right("neighbours", next(free), 150, (4,), a_subs=a_subs)
    # odd anchors: the window to the left; and pairs given the other way round (read A is the reverse mate)
    for edits in ((4,), (3, 1, 0), (5,)):
        left("left", next(free) + 200, 150, edits)
    for edits in ((3,), (2, 1, 1)):
        at = next(free)
        add("swapped", rc(substitute(rng, r0[at + 150:at + 150 + M], 2)), mutate(rng, r0, at, *edits), seq=0,
            anchor=(1, at + 150), found=(2, at), e=sum(edits), d=150)
    # mate A inside a tandem run of a 7-mer: a placement every 7 symbols, each an anchor of one query
    unit = A[rng.permutation(4)[[0, 1, 2, 3, 0, 2, 1]]]
    r0[22000:22000 + M + 70] = np.resize(unit, M + 70)
    bt = mutate(rng, r0, 22000 + 160, 3)
    add("tandem", substitute(rng, r0[22035:22035 + M], 1, 20, 28), rc(bt), seq=0, anchor=(0, 22035), found=(3, 22160), e=3,
        d=125)
    # dna5: an N in the mate against a base of the text, and against an N of the text
    right("N in mate", next(free), 150, (3,), n_at=21)
    r0[23000 + 150 + 18] = 4  # (no place of mutate's)
    right("N in both", 23000, 150, (3,))
    add("unmappable", substitute(rng, r0[24000:24000 + M], 2), A[rng.integers(0, 4, size=M)], seq=0, anchor=(0, 24000),
        found=None, e=None)
    # the bulk: rescuable pairs all over both records, and proper pairs that need nothing
    for i in range(24):
        rec = 1 if i % 6 == 0 else 0
        d = int(rng.integers(DMIN + 2, DMAX - 2))
        a = int(rng.integers(300, (19000 if rec == 0 else len(r1)) - d - M - 10))
        right("bulk", a, d, (3 + i % 4,) if i % 2 else (2 + i % 3, 1, i % 4 // 2), rec=rec)
    for i in range(10):
        a, d = int(rng.integers(300, 19000)), int(rng.integers(DMIN + 2, DMAX - 2))
        add("proper", substitute(rng, r0[a:a + M], i % 3), rc(substitute(rng, r0[a + d:a + d + M], 2 - i % 3)), seq=0,
            anchor=None, found=None, e=None)
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


_MODEL = {}


def model(setting, Kr, A=0, edit=True, rows=None, key="want"):
    """(rows of H u R, the stage's counts) for the oracle's rows, or for `rows` under the cache key `key`."""
    k = (setting, Kr, A, edit, key)
    if k not in _MODEL:
        c = planted()
        st = {}
        _MODEL[k] = (rescue(c["want"] if rows is None else rows, c["pats"], c["recs"], M, *setting, Kr, edit, A, st), st)
    return _MODEL[k]


def expect(setting, Kr, A=0, edit=True, rows=None, key="want"):
    """What a call returns: the pair rule over the rescued rows."""
    return pairs(model(setting, Kr, A, edit, rows, key)[0], M, *setting)


def added(setting, Kr, A=0):
    """The rescued records as a set of (qid, seq_id, pos, err)."""
    have = set(map(tuple, planted()["want"].tolist()))
    return set(map(tuple, model(setting, Kr, A)[0].tolist())) - have


@functools.lru_cache(maxsize=None)
def check():
    """What the GPU tests rely on, asserted on the model."""
    c = planted()
    w = c["want"]
    every = set(map(tuple, w[:, :3].tolist()))
    assert len(c["reads"]) % 2 == 0 and 150 <= len(c["reads"]) <= 200
    assert len(w) <= 20000
    for s in SETTINGS:
        idx, capped = anchors(w, c["recs"], M, *s, 0)
        assert len(idx) <= 150 and not capped, (s, len(idx))
        assert s[1] - max(s[0], M) + 1 <= 253
    idx, _ = anchors(w, c["recs"], M, *MAIN, 0)
    assert len(idx) >= 65, len(idx)  # more anchors than a wave has lanes, in the one batch of a call with SAHARA_BATCH unset
    assert [s[1] - max(s[0], M) + 1 for s in SETTINGS] == [253, 1, 63, 64, 65, 129]
    by = {}
    for e in c["plan"]:
        by.setdefault(e["kind"], []).append(e)

    def rec_of(e, which, err=None):
        q, p = e[which]
        return (4 * e["pair"] + q, e["seq"], p) + (() if err is None else (err,))

    R = {Kr: added(MAIN, Kr) for Kr in (2,) + KS}
    assert not R[2]  # K <= k adds nothing
    for Kr in KS:
        assert all(K < r[3] <= Kr for r in R[Kr]), Kr
    for e in c["plan"]:
        if e["anchor"] is None:
            continue
        assert rec_of(e, "anchor") in every, e["kind"]
        if e["found"] is not None:  # the mate did not map
            assert not any(r[0] == 4 * e["pair"] + e["found"][0] for r in every), e["kind"]
        for Kr in KS:
            mine = {r for r in R[Kr] if r[0] // 4 == e["pair"]}
            if e["e"] is not None and e["e"] <= Kr:
                assert mine == {rec_of(e, "found", e["e"])}, (e["kind"], Kr, mine, e)
            elif not e.get("shifted"):
                assert not mine, (e["kind"], Kr, mine)
    assert {e["e"] for e in by["errors"]} == {3, 4, 5, 8}
    # one start outside the window: nothing at K = 3; a shifted placement at 5 errors from K = 5 on
    for kind in ("below lo", "above hi"):
        for e in by[kind]:
            assert not {r for r in R[3] if r[0] // 4 == e["pair"]}, kind
            if e.get("shifted"):
                mine = {r for r in R[8] if r[0] // 4 == e["pair"]}
                assert len(mine) == 1 and min(mine)[3] > 3 and min(mine)[2] != e["found"][1], (kind, mine)
    # the narrow settings: the round-edge mates are inside or outside by their index
    for s in (ONE, W63, W64, W65, W129):
        dmin, dmax = max(s[0], M) - M, s[1] - M
        got = added(s, 3)
        for e in by["round edge"]:
            assert (rec_of(e, "found", 3) in got) == (dmin <= e["d"] <= dmax), (s, e["d"])
        assert got, s
    assert sorted(e["d"] - DMIN for e in by["round edge"]) == [62, 63, 64, 100, 128]
    for e in by["clipped at end"]:
        assert e["anchor"][1] + DMAX > len(c["recs"][e["seq"]]) - 1
        assert e["found"][1] == len(c["recs"][e["seq"]]) - M  # the last placement that fits
    for e in by["clipped at 0"]:
        assert e["anchor"][1] < DMAX and e["found"][1] in (0, 2)
    assert any(e["found"][1] == 0 for e in by["clipped at 0"])
    # equal copies: the smaller start; unequal ones: the cheaper, wherever it lies
    for kind in ("tie in a round", "tie across rounds", "cheaper later", "dearer later"):
        e, = by[kind]
        rec, lo = c["recs"][0], e["anchor"][1] + DMIN
        pat = c["pats"][4 * e["pair"] + 3]
        for at, err in (e["found"][1], e["e"]), e["other"]:
            assert scan(rec, pat, at, at, 8, True) == (err, at), kind
        first, second = sorted((e["found"][1] - lo, e["other"][0] - lo))
        assert (first // 64 == second // 64) == (kind == "tie in a round"), kind
        if kind.startswith("tie"):
            assert e["found"][1] < e["other"][0] and e["e"] == e["other"][1]
        else:
            assert e["e"] < e["other"][1] and (e["found"][1] > e["other"][0]) == (kind == "cheaper later")
            assert e["other"][1] <= 5  # found in an earlier round at K = 5 and 8, then beaten
    # duplicates at the anchor's position, and anchors at p +- 1 that find the same record
    idx_set = set(map(tuple, w[idx][:, :3].tolist()))
    for e in by["neighbours"]:
        q, s, p = rec_of(e, "anchor")
        near = {r for r in idx_set if r[0] == q}
        if e is by["neighbours"][0]:
            assert {(q, s, p - 1), (q, s, p), (q, s, p + 1)} <= near
            assert sum(1 for r in w[:, :3].tolist() if tuple(r) == (q, s, p)) >= 2
    assert sum(1 for r in idx_set if r[0] % 2 == 1) >= 5  # odd anchors
    # the tandem query: more anchors than the cap
    e, = by["tandem"]
    q = 4 * e["pair"]
    mine = [r for r in idx_set if r[0] == q]
    assert CAP < len(mine) <= 32, len(mine)
    capped = anchors(w, c["recs"], M, *MAIN, CAP)[1]
    assert capped == [q], capped
    for Kr in KS:
        assert added(MAIN, Kr) - added(MAIN, Kr, CAP) == {rec_of(e, "found", 3)}, Kr
    for kind in ("N in mate", "N in both"):
        e, = by[kind]
        assert (c["pats"][4 * e["pair"] + 3] == 4).sum() == 1, kind
    e, = by["N in both"]
    assert c["recs"][0][e["found"][1] + 18] == 4 and c["pats"][4 * e["pair"] + 3][18] == 4
    # every K keeps more than the one below it, and all more than the pair rule alone
    sizes = {Kr: len(expect(MAIN, Kr)) for Kr in KS}
    assert len(pairs(w, M, *MAIN)) < sizes[3] < sizes[5] < sizes[8], sizes
    return c
