"""The grid of the paired chain's tests: the planted cases of the pair, rescue,
best-pairs and links tests all sit at M = 48, sigma = 6, K = 2 on two long
records; case(point) builds a small world at another pattern length, alphabet,
error bound and fragment range, on some forty records of which most are
shorter than a window, a fragment or the pattern. check(point) asserts on the
CPU, through the models over the oracle's rows, that the point still covers
the edge it is in GRID for. No GPU: tests/test_paired_grid_gpu.py runs it on
one.

The records: one of 6000 symbols; forty short ones of the lengths 1, M - 1,
M, M + 1, 2M, min_fragment, min_fragment + 1, max_fragment and 3M + 7 in turn,
the second and third of each length copies of the first (a pair on one of
them has its placements on several seq_ids, which the pair rule's and the
links' (qid, seq_id, pos) comparisons have to tell apart; at M = 250, where
the pairs are few, the fourth too); a last one that holds a full window and
is followed by the text's end pad.

The pairs (plan[i]["kind"]): "out" (one each at d = dmin - 1 and dmax + 1),
"end" (the reverse mate ends 0, 1 and K symbols before its record's last, the
forward mate as close to it as dmin allows: at the same position where dmin
is 0), "across" (a forward anchor whose mate would continue behind its
record's '$'), "lonely" (a mate that is a whole record of M symbols, or one
of M - 1 symbols with a symbol put in: records on which no fragment fits),
and the bulk, made like pairs_case.proper: half found by the search, half
with K + 1 .. Kr edits in one mate (rescue_case.mutate's), every seventh
given the other way round, two thirds on the short records. The rescued mate
is mate B, but for every fourth pair, where it is mate A: with the pairs
given the other way round these are the odd-qid anchors, their windows
clipped at position 0. The widest window has more, all on the last record:
"index" (the rescued mate at window index 0, 4031, 4032 and 4095), "tie
across rounds" and "cheaper later" (rescue_case's copies, in rounds 0 and
63) and "wide" (full windows of 4096 starts).

CPU time of one point, the oracle's search and every model that check()
asks, in seconds as measured where this was written: M = 20: 0.1, 32: 0.1,
33: 1.5, 64: 0.3, 65: 0.1, 100: 1.1, 250: 2.3 (16 pairs; 60 took 11 s in a
sketch of this generator), 64 Hamming: 0.1.
"""
import functools
from typing import NamedTuple

import numpy as np

import oracle as O
import sahara_amd as sa
from helpers import acgt, hits_as_rows
from loci_model import loci
from pair_links_model import pair_links
from pairs_model import pairs
from rescue_model import anchors, rescue, window
from test_golden import RC


class Point(NamedTuple):
    M: int
    sigma: int
    K: int
    generator: str
    frag: tuple  # (min_fragment, max_fragment)
    Kr: int
    edit: bool


GRID = (
    Point(20, 5, 1, "h2-k1", (30, 90), 3, True),          # one pattern block
    Point(32, 6, 2, "h2-k2", (40, 200), 5, True),         # fills its block exactly
    Point(33, 5, 2, "h2-k2", (33, 33 + 4095), 4, True),   # one past a block; the widest window; dmin = 0
    Point(64, 6, 2, "h2-k2", (100, 400), 8, True),        # two full blocks, the largest Kr
    Point(65, 5, 1, "h2-k1", (65, 300), 3, True),         # min_fragment == len
    Point(100, 6, 3, "pigeon", (150, 500), 6, True),      # K = 3, four blocks
    Point(250, 5, 2, "h2-k2", (300, 700), 5, True),       # eight blocks; 16 pairs
    Point(64, 6, 2, "h2-k2", (100, 400), 5, False),       # the scan without indels
)
WIDEST = GRID[2]
MAX_WINDOW = 4096
# what each point is in the grid for: (pattern blocks, symbols in the last block)
BLOCKS = {20: (1, 20), 32: (1, 32), 33: (2, 1), 64: (2, 32), 65: (3, 1), 100: (4, 4), 250: (8, 26)}
# the widest point's extra pairs on the last record: (anchor position, window index of the rescued mate)
INDEX_PAIRS = ((40, 0), (140, 4031), (240, 4032), (340, 4095))
# ... and its copies: (anchor, index of the first copy, of the second, extra substitutions in the first)
COPY_PAIRS = (("tie across rounds", 440, 40, 4040, 0), ("cheaper later", 540, 40, 4050, 1))
WIDE_PAIRS = 12  # ... and those with a full window of 4096 starts each


def name(point):
    return f"M{point.M}-sigma{point.sigma}-K{point.K}-{'lev' if point.edit else 'ham'}{point.Kr}"


def dists(point):
    """(dmin, dmax): the least and the largest distance of the mates' starts."""
    return max(point.frag[0], point.M) - point.M, point.frag[1] - point.M


def total_pairs(point):
    return 16 if point.M >= 250 else 60  # (at M = 250 sixty pairs cost the oracle and the models some 11 s)


def rc(x, sigma):
    return RC[sigma][np.asarray(x, np.uint8)][::-1]


def substitute(rng, x, n, sigma):
    """n substitutions at distinct inner places (pairs_case.substitute at any length)."""
    x = np.array(x, np.uint8)
    A = acgt(sigma)
    for j in rng.choice(np.arange(3, len(x) - 3), size=n, replace=False):
        x[j] = rng.choice(A[A != x[j]])
    return x


def mutate(rng, r, b, M, sigma, subs, ins=0, dele=0, with_n=False):
    """rescue_case.mutate at any length: a pattern of M symbols that fits r at
    b with subs + ins + dele edits at distinct inner places 2 to 4 apart;
    with_n: one of the substitutions is an N. A deletion that the record's end
    leaves no text for becomes a substitution."""
    A = acgt(sigma)
    if b + M + dele - ins > len(r):
        subs, dele = subs + dele, 0
    n = subs + ins + dele
    t = list(np.asarray(r[b:b + M + dele - ins], np.uint8))
    step = min(4, (M - 6) // max(n, 1))
    assert step >= 2 and len(t) == M + dele - ins
    places = 3 + step * rng.permutation((M - 6) // step)[:n]
    kinds = ["X"] * subs + ["I"] * ins + ["D"] * dele
    n_at = int(places[0]) if with_n else None
    for at, kind in sorted(zip(places.tolist(), kinds), reverse=True):  # from the right: places stay put
        if kind == "D":
            del t[at]
        elif kind == "I":
            t.insert(at, int(rng.choice(A[(A != t[at]) & (A != t[at - 1])])))
        else:
            t[at] = 4 if at == n_at else int(rng.choice(A[A != t[at]]))
    assert len(t) == M
    return np.array(t, np.uint8)


def short_lengths(point):
    M, (fmin, fmax) = point.M, point.frag
    return (1, M - 1, M, M + 1, 2 * M, fmin, fmin + 1, fmax, 3 * M + 7)


N_SHORT, N_LENGTHS = 40, 9


def records(rng, point):
    """(the records, seq_ids of the short records with copies that hold a pair, of those without)."""
    M = point.M
    dmin, dmax = dists(point)
    A = acgt(point.sigma)

    def random(n):
        return A[rng.integers(0, 4, size=n)].astype(np.uint8)

    lens = short_lengths(point)
    copies = 3 if M >= 250 else 2  # (M = 250 has few pairs: each rescued mate is needed on four records)
    recs = [random(6000)]
    for j in range(N_SHORT):
        recs.append(recs[1 + j % N_LENGTHS].copy() if 1 <= j // N_LENGTHS <= copies else random(lens[j % N_LENGTHS]))
    recs.append(random(dmax + M + 800))
    if point.sigma == 6:
        recs[0][3000:3003] = 4  # a few N in one record
    holds = [1 + j for j in range(N_SHORT) if lens[j % N_LENGTHS] >= dmin + M + 1]
    copied = [s for s in holds if (s - 1) // N_LENGTHS == 0]
    single = [s for s in holds if (s - 1) // N_LENGTHS > copies]
    return recs, copied, single or copied


@functools.lru_cache(maxsize=None)
def case(point):
    M, sigma, K, Kr = point.M, point.sigma, point.K, point.Kr
    dmin, dmax = dists(point)
    rng = np.random.default_rng(1000 * M + 10 * sigma + point.edit)
    A = acgt(sigma)
    recs, copied, single = records(rng, point)
    last = len(recs) - 1
    mates, plan = [], []

    def add(kind, fwd, rev, seq, a, b, swapped=False, **what):
        """fwd: the forward mate (the text at a), rev: the reverse one (the reverse
        complement of the text at b). Given the other way round, read A is the
        reverse mate: its reverse complement, an odd qid, lies at b."""
        fwd, rev = np.asarray(fwd, np.uint8), np.asarray(rev, np.uint8)
        plan.append(dict(kind=kind, pair=len(mates), seq=seq, a=a, b=b, fq=2 if swapped else 0, rq=1 if swapped else 3,
                         **what))
        mates.append((rev, fwd) if swapped else (fwd, rev))

    def exact(seq, at):  # K substitutions: nothing but the exact position lies within K errors
        return substitute(rng, recs[seq][at:at + M], K, sigma)

    # the widest window: the copies first, they change the last record's text
    if point == WIDEST:
        r = recs[last]
        assert len(r) >= COPY_PAIRS[-1][1] + COPY_PAIRS[-1][3] + M + Kr
        for kind, at, d1, d2, extra in COPY_PAIRS:
            seg = r[at + d1:at + d1 + M].copy()
            r[at + d2:at + d2 + M] = seg
            for j in (1, M - 2)[:extra]:  # (outside the places substitute() changes)
                r[at + d1 + j] = A[(np.flatnonzero(A == seg[j])[0] + 1) % 4]
            add(kind, exact(last, at), rc(substitute(rng, seg, K + 1, sigma), sigma), last, at, at + d2, rescue=True,
                other=at + d1, extra=extra)
        for at, index in INDEX_PAIRS:
            add("index", exact(last, at), rc(mutate(rng, r, at + index, M, sigma, K + 1), sigma), last, at, at + index,
                rescue=True, index=index)
        # and full windows, so that the call scans more starts than 64 anchors' worth: a forward mate as the
        # text has it is an anchor at its position and at the ones beside it
        for i in range(WIDE_PAIRS):
            at, d = 650 + 14 * i, 900 + 200 * i
            add("wide", r[at:at + M].copy(), rc(substitute(rng, r[at + d:at + d + M], K + 1, sigma), sigma), last, at,
                at + d, rescue=True)
    extra = len(mates)
    # one start outside the window on either side, each mate with its only hit
    for at, d in ((500, dmin - 1), (700, dmax + 1)):
        add("out", exact(0, at), rc(exact(0, at + d), sigma), 0, at, at + d, rescue=False)
    # the reverse mate 0, 1 and K symbols before its record's last, the forward one as close as dmin allows
    # (all three for the rescue: its scan is what reads the text there)
    for seq, t in ((last, 0), (copied[-1], 1), (copied[-2], K)):
        b = len(recs[seq]) - M - t
        add("end", exact(seq, b - dmin), rc(mutate(rng, recs[seq], b, M, sigma, K + 1), sigma), seq, b - dmin, b,
            rescue=True)
    # a forward anchor whose window starts on its record and whose mate would run on behind the '$': record 0 is
    # followed by the record of one symbol, the last one by the text's end
    d = max(dmin, M - M // 2)
    for seq in (0, copied[0], last):
        b = len(recs[seq]) - M // 2
        behind = np.concatenate([recs[seq][b:]] + recs[seq + 1:seq + 12] + [A[rng.integers(0, 4, size=M)]])[:M]
        add("across", exact(seq, b - d), rc(behind, sigma), seq, b - d, b, rescue=False)
    # records on which no fragment fits: a mate that is the whole record of M symbols, and one that is the
    # record of M - 1 symbols with a symbol put in (search and scan with indels only)
    add("lonely", recs[3].copy(), A[rng.integers(0, 4, size=M)], 3, 0, 0, rescue=False)
    if point.edit:
        r = recs[2]
        add("lonely", np.insert(r, M // 2, A[(np.flatnonzero(A == r[M // 2])[0] + 1) % 4]), A[rng.integers(0, 4, size=M)],
            2, 0, 0, rescue=False)
    # the bulk
    n_found = n_rescue = 0
    for i in range(total_pairs(point) + extra - len(mates)):
        rescued, swapped = i % 2 == 1, i % 7 == 1
        left = rescued and i % 4 == 3 and not swapped  # the forward mate is the one to rescue: an odd anchor
        if i % 3:
            seq = int(rng.choice(copied if rescued else single))
        else:
            seq = (0, last)[i // 3 % 2]
        r = recs[seq]
        room = len(r) - M - dmin  # the largest a
        a = int(rng.integers(0, min(room, M) + 1 if left else room + 1))
        most = min(dmax, len(r) - M - a)
        if left:  # b < dmax: the odd anchor's window is clipped at position 0
            d = int(rng.integers(dmin, max(dmin, min(most, dmax - a - 1)) + 1))
        elif i % 10 == 0:
            d = dmin if i // 10 % 2 == 0 else most
        else:
            d = int(rng.integers(dmin, most + 1))
        b = a + d
        light = substitute(rng, r[(b if left else a):(b if left else a) + M], i % (K + 1), sigma)
        if rescued:
            e = K + 1 + n_rescue % (Kr - K)
            ins = 1 if point.edit and n_rescue % 2 == 0 else 0
            dele = 1 if ins and n_rescue // 2 % 2 and e >= 2 else 0
            heavy = mutate(rng, r, a if left else b, M, sigma, e - ins - dele, ins, dele,
                           with_n=sigma == 6 and n_rescue == 1)
            n_rescue += 1
        else:
            heavy = substitute(rng, r[b:b + M], n_found % (K + 1), sigma)
            n_found += 1
        fwd, rev = (heavy, light) if left else (light, heavy)
        add("bulk", fwd, rc(rev, sigma), seq, a, b, swapped=swapped, rescue=rescued, left=left, d=d)
    order = rng.permutation(len(mates))
    where = np.argsort(order)  # pair `p` of the plan is pair where[p] of the reads
    for e in plan:
        e["pair"] = int(where[e["pair"]])
    reads = np.ascontiguousarray(np.stack([m for i in order for m in mates[i]]).astype(np.uint8))
    pats = sa.interleave_rc(reads, sigma)
    scheme = sa.search_scheme(point.generator, 0, K, M, hamming=not point.edit)
    ref = O.Index.build(recs, sigma, 16)
    want = hits_as_rows(ref.search(pats, scheme, edit=point.edit, nthreads=8)[0])
    return dict(point=point, sigma=sigma, recs=recs, reads=reads, pats=pats, scheme=scheme, ref=ref, want=want, plan=plan,
                n_pairs=len(mates))


@functools.lru_cache(maxsize=None)
def rows_in(point, W=None):
    """The rows the chain starts from: the oracle's, or with loci on their representatives."""
    w = case(point)["want"]
    return w if W is None else loci(w, W)


@functools.lru_cache(maxsize=None)
def rescued(point, W=None):
    """(the rows of H u R, the rescue's counts) of the model."""
    c = case(point)
    st = {}
    return rescue(rows_in(point, W), c["pats"], c["recs"], point.M, *point.frag, point.Kr, point.edit, 0, st), st


@functools.lru_cache(maxsize=None)
def links(point, delta, W=None):
    """(kept rows, summary, links, info) of the model over the rescued rows."""
    return pair_links(rescued(point, W)[0], point.M, *point.frag, delta, case(point)["n_pairs"])


@functools.lru_cache(maxsize=None)
def check(point):
    """What the GPU tests rely on, and what the point is in the grid for, asserted on the models."""
    c = case(point)
    M, sigma, K, Kr = point.M, point.sigma, point.K, point.Kr
    dmin, dmax = dists(point)
    recs, pats, w, plan = c["recs"], c["pats"], c["want"], c["plan"]
    lens = [len(r) for r in recs]
    last = len(recs) - 1
    # the point's edge: block count and fill, alphabet, window
    assert pats.shape[1] == M and (-(-M // 32), (M - 1) % 32 + 1) == BLOCKS[M]
    assert set(np.unique(np.concatenate(recs)).tolist()) == set(range(1, sigma))
    assert int(pats.max()) == sigma - 1  # rank 4 is T with sigma = 5, N with sigma = 6
    if sigma == 6:
        n_text = [s for s, r in enumerate(recs) if (r == 4).any()]
        n_mates = [q for q in range(0, len(pats), 2) if (pats[q] == 4).any()]
        assert n_text == [0] and len(n_mates) == 1, (n_text, n_mates)
    assert dmax - dmin < MAX_WINDOW and (dmax - dmin == MAX_WINDOW - 1) == (point == WIDEST)
    assert (dmin == 0) == (point.frag[0] <= M) == (M in (33, 65))
    assert c["n_pairs"] == total_pairs(point) + (len(INDEX_PAIRS) + len(COPY_PAIRS) + WIDE_PAIRS if point == WIDEST else 0)
    # the records: shorter than the pattern, too short for a fragment, copies, a last one that holds a window
    assert len(recs) == N_SHORT + 2 and sorted(set(lens[1:-1])) == sorted(set(short_lengths(point)))
    assert min(lens) == 1 and M - 1 in lens and lens[last] > dmax + 2 * M
    assert all(np.array_equal(recs[s], recs[s + N_LENGTHS]) for s in range(1, 1 + N_LENGTHS))
    small = {s for s, n in enumerate(lens) if n < dmin + M}  # no fragment fits
    on = set(w[:, 1].tolist())
    assert any(lens[s] == M for s in on) and (not point.edit or any(lens[s] == M - 1 for s in on)), sorted(on)
    # the chain
    kept_pairs = pairs(w, M, *point.frag)
    rows, st = rescued(point)
    have = set(map(tuple, w.tolist()))
    new = [tuple(r) for r in rows.tolist() if tuple(r) not in have]
    assert len(new) == st["rescued"] >= 20 and all(K < r[3] <= Kr for r in new), (len(new), st)
    assert {e for _, _, _, e in new} == set(range(K + 1, Kr + 1))  # every error count the scan may report
    idx, capped = anchors(w, recs, M, *point.frag, 0)
    assert not capped and st["anchors"] == len(idx)
    odd = clipped_end = clipped_0 = 0
    for q, s, p, _ in w[idx].tolist():
        lo, hi = window(q, p, dmin, dmax, lens[s])
        odd += q % 2
        clipped_end += q % 2 == 0 and hi < p + dmax
        clipped_0 += q % 2 == 1 and lo > p - dmax
    assert odd >= 5 and clipped_end >= 1 and clipped_0 >= 1, (odd, clipped_end, clipped_0)
    by = {}
    for e in plan:
        by.setdefault(e["kind"], []).append(e)
    every = set(map(tuple, w[:, :3].tolist()))
    anchor_at = set(map(tuple, w[idx][:, :3].tolist()))

    def fwd(e):
        return (4 * e["pair"] + e["fq"], e["seq"], e["a"])

    def rev(e):
        return (4 * e["pair"] + e["rq"], e["seq"], e["b"])

    def of_pair(rows_, e):
        return [r for r in rows_ if r[0] // 4 == e["pair"]]

    # one start outside the window: both mates map, the pair rule keeps neither, and what the rescue may add to
    # the pair is a shifted placement of more than K errors, never the planted one
    assert [e["b"] - e["a"] for e in by["out"]] == [dmin - 1, dmax + 1]
    for e in by["out"]:
        assert fwd(e) in every and rev(e) in every and not of_pair(kept_pairs.tolist(), e), e
        assert all(r[:3] != rev(e) and r[:3] != fwd(e) for r in of_pair(new, e)), e
    # at a record's end: the reverse mate's m + K symbols reach the '$'; where dmin <= K + 1 both mates lie there
    assert len(by["end"]) == 3
    for e in by["end"]:
        assert e["b"] + M + K >= lens[e["seq"]] and e["b"] - e["a"] == dmin
        got = rev(e) + (K + 1,) in new if e["rescue"] else rev(e) in every
        assert got and fwd(e) in every, e
    assert any(e["rescue"] and e["seq"] == last for e in by["end"])  # (the scan reads the text's end pad)
    # across the '$': an anchor with a window, nothing found
    assert len(by["across"]) == 3 and lens[by["across"][0]["seq"] + 1] == 1 and by["across"][-1]["seq"] == last
    for e in by["across"]:
        assert fwd(e) in anchor_at and e["a"] + dmin <= lens[e["seq"]] - 1 < e["b"] + M - 1 and not of_pair(new, e), e
    # records on which no fragment fits keep nothing, with hits on them
    kept0, summary0, links0, info0 = links(point, 0)
    assert small & on and not small & set(kept0[:, 1].tolist())
    for e in by["lonely"]:
        assert (4 * e["pair"], e["seq"], 0) in every and lens[e["seq"]] in (M, M - 1), e
    # kept hits all over the records, on copies too; ties and lone placements
    seqs = set(kept0[:, 1].tolist())
    assert len(seqs) >= 10 and any(s + N_LENGTHS in seqs for s in seqs if 1 <= s <= N_LENGTHS), sorted(seqs)
    mapq = {int(x) for x in links0["mapq"][links0["flags"] != 0]}
    assert info0["n_best"].max() >= 2 and 60 in mapq, (info0["n_best"].max(), mapq)
    for delta in (0, 1):
        k, summary, ln, info = links(point, delta)
        assert len(ln) >= 60 or M >= 250, len(ln)
        assert len(set(map(tuple, k.tolist())) & set(new)) >= 15  # the links run over rescued records
    assert len(links(point, 1)[0]) >= len(kept0)
    if point == WIDEST:
        # the rescued mate at the last round's first and last lane, at the anchor's own position, one before
        # the last round; the copies in rounds 0 and 63
        for e in by["index"]:
            assert e["seq"] == last and rev(e) + (K + 1,) in new and e["b"] - (e["a"] + dmin) == e["index"], e
        assert sorted(e["index"] for e in by["index"]) == [0, 4031, 4032, 4095]
        assert by["index"][0]["a"] == by["index"][0]["b"]  # (dmin = 0: the mate at the anchor's position)
        (tie,), (cheaper,) = by["tie across rounds"], by["cheaper later"]
        for e in (tie, cheaper):
            assert (e["other"] - e["a"]) // 64 == 0 and (e["b"] - e["a"]) // 64 == 63
        assert (4 * tie["pair"] + 3, last, tie["other"], K + 1) in new and not rev(tie) + (K + 1,) in new
        assert rev(cheaper) + (K + 1,) in new and K + 1 + cheaper["extra"] <= Kr  # (round 0 finds the dearer one first)
        assert st["starts"] > 64 * MAX_WINDOW, st
    return c
