"""Inputs at the ends of the range the library accepts (CPU only: numpy and
the oracle): searches with 5 to 15 errors, scheme tables at the limits of
staging.cpp (255 searches, searches * len = 15360), 16 besthits rounds and
patterns of thousands of symbols.

Every builder is seeded, runs once per process (lru_cache) and returns a dict:
records, reads, the patterns the oracle searched (`pats`: the reads themselves,
or with `reverse` their interleave with the reverse complements), the
scheme(s), the oracle's sorted (qid, seq_id, pos, e) rows over its own index of
the records (`want`), the set of error counts the case exists for (`errs`) and
the oracle's wall time (`oracle_s`). tests/test_range_inputs.py asserts what
each case is for without a GPU; tests/test_range_ends.py runs them on one.
"""
import functools
import time

import numpy as np

import oracle as O
from helpers import acgt, hits_as_rows, mutate_reads, random_records, substituted_reads

ORACLE_THREADS = 8
ORACLE_CAP_S = 10.0  # a case whose oracle call takes longer fails test_range_inputs.py


def interleave_rc(reads, sigma):
    """qid 2i = read i, 2i + 1 = its reverse complement (N stays N)."""
    comp = np.arange(8, dtype=np.uint8)
    comp[acgt(sigma)] = acgt(sigma)[::-1]
    out = np.empty((2 * len(reads), reads.shape[1]), np.uint8)
    out[0::2] = reads
    out[1::2] = comp[reads[:, ::-1]]
    return out


def record_ends(recs, m):
    """Every long-enough record's first and last m symbols."""
    long_enough = [r for r in recs if len(r) >= m]
    return np.stack([r[:m] for r in long_enough] + [r[-m:] for r in long_enough])


def edits_by_classes(rng, recs, n, m, k, sigma):
    """n reads with 0..k random S/I/D, read i with i % (k + 1) of them."""
    out = np.zeros((n, m), np.uint8)
    for e in range(k + 1):
        rows = np.arange(e, n, k + 1)
        if len(rows):
            out[rows] = mutate_reads(rng, recs, len(rows), m, e, sigma)
    return out


def _timed(call):
    t = time.perf_counter()
    rows = call()
    return hits_as_rows(rows), time.perf_counter() - t


def _search_case(name, sigma, edit, k, recs, reads, scheme, errs, reverse=False):
    pats = interleave_rc(reads, sigma) if reverse else reads
    pats = np.ascontiguousarray(pats)
    ref = O.Index.build(recs, sigma, 16)
    want, dt = _timed(lambda: ref.search(pats, scheme, edit=edit, nthreads=ORACLE_THREADS)[0])
    return dict(name=name, sigma=sigma, edit=edit, k=k, m=reads.shape[1], recs=recs,
                reads=np.ascontiguousarray(reads), pats=pats, reverse=reverse, scheme=scheme, want=want,
                errs=set(errs), oracle_s=dt)


# ------------------------------------------- a. Hamming up to 15 errors ----

HAMMING = {  # name: (generator, k, m, sigma, searches the generator gives)
    "pigeon-k15": ("pigeon", 15, 40, 6, 16),
    "backtracking-k15": ("backtracking", 15, 64, 5, 1),
    "h2-k2-k8": ("h2-k2", 8, 40, 6, 15),
    "pex-bu-l-k7": ("pex-bu-l", 7, 33, 6, None),
}


@functools.lru_cache(maxsize=None)
def hamming(name, reverse=False):
    """100 reads on [3000, 1500] (an N run and repeats): 96 with i % (k + 1)
    substitutions, then the records' first and last m symbols."""
    gen, k, m, sigma, nsearch = HAMMING[name]
    rng = np.random.default_rng(1000 * m + 10 * k + sigma)
    recs = random_records(rng, [3000, 1500], sigma, with_n=True, repeats=True)
    reads = np.vstack([substituted_reads(rng, recs, 96, m, k, sigma), record_ends(recs, m)])
    scheme = O.scheme(gen, 0, k, m, hamming=True)
    assert nsearch is None or len(scheme[0]) == nsearch, (name, len(scheme[0]))
    return _search_case(name + ("-rc" if reverse else ""), sigma, False, k, recs, reads, scheme, range(k + 1), reverse)


# ------------------------- b. edit distance, all-mode, k = 5 to 8 ----------

EDIT = {  # name: (generator, k, m, sigma, record lengths, reads)
    "pigeon-k5": ("pigeon", 5, 24, 6, (600, 300), 40),
    "pigeon-k6": ("pigeon", 6, 28, 5, (400, 200), 30),
    # a read with no edit alone has about a million rows at k = 7 and 8 (every
    # way to spend the slack is a row): one read per error count
    "pigeon-k7": ("pigeon", 7, 32, 6, (400, 200), 10),
    "pex-bu-k8": ("pex-bu", 8, 36, 6, (400, 200), 11),
}


def substituted_ends(rng, recs, m, k, sigma):
    """Record 0's first and the last record's last m symbols, k substitutions
    inside each: hits of k errors at a record's first and last symbol without
    the rows of a read that leaves the whole bound as slack."""
    alpha = acgt(sigma)
    out = np.stack([recs[0][:m], recs[-1][-m:]])
    for s in out:
        for j in rng.choice(np.arange(1, m - 1), size=k, replace=False):
            s[j] = rng.choice(alpha[alpha != s[j]])
    return out


@functools.lru_cache(maxsize=None)
def edit(name):
    """Reads with 0..k edits by classes, the last two at the records' ends. The
    rows are path multiplicities: up to a million per query, a few hundred
    distinct positions."""
    gen, k, m, sigma, lengths, n = EDIT[name]
    rng = np.random.default_rng(1000 * m + 10 * k + sigma + 1)
    recs = random_records(rng, list(lengths), sigma, with_n=True)
    reads = np.vstack([edits_by_classes(rng, recs, n - 2, m, k, sigma), substituted_ends(rng, recs, m, k, sigma)])
    return _search_case(name, sigma, True, k, recs, reads, O.scheme(gen, 0, k, m), range(k + 1))


# ------------------- c. edit distance up to 15 errors: staircase schemes ----

def staircase_scheme(m, parts, lag):
    """Two searches, left to right and right to left, over `parts` equal parts:
    part p (in search order) has u = min(p, 15); l is max(p - lag, 0) at the
    part's last position and the previous part's l inside it. Valid (l <= u,
    both monotone, connected orders), not complete: a read is found by the
    search whose order meets the read's edits no faster than one per part."""
    size = m // parts
    assert size * parts == m
    p = np.arange(parts)
    last = np.maximum(p - lag, 0)
    inside = np.concatenate([[0], last[:-1]])
    l = np.repeat(inside, size)
    l[size - 1::size] = last
    u = np.repeat(np.minimum(p, 15), size)
    order = np.arange(m)
    as_u32 = lambda rows: np.ascontiguousarray(np.stack(rows), dtype=np.uint32)
    return as_u32([order, order[::-1]]), as_u32([l, l]), as_u32([u, u])


def staircase_reads(rng, recs, n, m, parts, sigma, lag=1):
    """Read i has one edit (S, I, D cycling) strictly inside every part but the
    first (even i: the left-to-right search finds it) or the last (odd i: the
    right-to-left one); pairs of reads in turn leave 1 .. lag + 1 parts clean,
    so every error count from the last lower bound to 15 is met. Read 0 starts
    at position 0 of record 0, read 1 ends at record 0's last symbol."""
    size = m // parts
    alpha = acgt(sigma)
    out = np.zeros((n, m), np.uint8)
    for i in range(n):
        n_clean = 1 + (i // 2) % (lag + 1)
        clean = range(n_clean) if i % 2 == 0 else range(parts - n_clean, parts)
        kinds = [None if q in clean else "SID"[(i + q) % 3] for q in range(parts)]
        used = m + kinds.count("D") - kinds.count("I")  # text symbols the read is made of
        r = recs[0] if i < 2 else recs[rng.integers(len(recs))]
        t = 0 if i == 0 else len(r) - used if i == 1 else int(rng.integers(0, len(r) - used + 1))
        segs = []
        for kind in kinds:
            j = int(rng.integers(1, size - 1))
            if kind is None:
                seg, step = r[t:t + size].copy(), size
            elif kind == "S":
                seg, step = r[t:t + size].copy(), size
                seg[j] = rng.choice(alpha[alpha != seg[j]])
            elif kind == "I":  # a read symbol the text does not have
                seg, step = np.concatenate([r[t:t + j], [rng.choice(alpha)], r[t + j:t + size - 1]]), size - 1
            else:              # a text symbol the read does not have
                seg, step = np.concatenate([r[t:t + j], r[t + j + 1:t + size + 1]]), size + 1
            assert len(seg) == size
            segs.append(seg)
            t += step
        out[i] = np.concatenate(segs)
    return out


STAIRCASE = {  # name: (m, parts, lag, sigma)
    "m96-lag1-dna5": (96, 16, 1, 6),
    "m128-lag2-dna4": (128, 16, 2, 5),
}


@functools.lru_cache(maxsize=None)
def staircase(name):
    m, parts, lag, sigma = STAIRCASE[name]
    rng = np.random.default_rng(17 * m + lag + sigma)
    recs = random_records(rng, [600, 300], sigma, with_n=True, repeats=True)
    reads = staircase_reads(rng, recs, 20, m, parts, sigma, lag)
    scheme = staircase_scheme(m, parts, lag)
    return _search_case(name, sigma, True, 15, recs, reads, scheme, range(15 - lag, 16))


# ------------------------------------------ d. besthits over 16 rounds ----

def best_round_scheme(m, parts, j):
    """Round j: one left-to-right search in which each of the last j parts
    admits one more error. In such a part u = c, the errors admitted so far, l
    is c - 1 inside it and c at its last position; l = j at the very end."""
    size = m // parts
    c = np.maximum(np.arange(parts) - (parts - j) + 1, 0)
    u = np.repeat(c, size)
    l = np.repeat(np.maximum(c - 1, 0), size)
    l[size - 1::size] = c
    assert l[-1] == j and (l <= u).all()
    as_u32 = lambda row: np.ascontiguousarray(row[None, :], dtype=np.uint32)
    return as_u32(np.arange(m)), as_u32(l), as_u32(u)


TWIN = 300  # best16: 160 symbols from here in record 0 stand in record 1 as well


@functools.lru_cache(maxsize=None)
def best16():
    """32 reads of 96 symbols, two per error count j = 0..15, one substitution
    strictly inside each of the last j of 16 parts; the first starts a record,
    the second ends one."""
    m, parts, sigma = 96, 16, 6
    size = m // parts
    rng = np.random.default_rng(1696)
    recs = random_records(rng, [600, 300], sigma, with_n=True, repeats=True)
    recs[1][100:260] = recs[0][TWIN:TWIN + 160]  # every fourth read comes from here: found at two positions
    alpha = acgt(sigma)
    reads = np.zeros((32, m), np.uint8)
    for i in range(32):
        r = recs[i % 2]
        t = 0 if i == 0 else len(r) - m if i == 1 else int(rng.integers(0, len(r) - m + 1))
        if i % 4 == 2:
            t = TWIN + int(rng.integers(0, 160 - m + 1))
        s = r[t:t + m].copy()
        for q in range(parts - i // 2, parts):
            j = q * size + int(rng.integers(1, size - 1))
            s[j] = rng.choice(alpha[alpha != s[j]])
        reads[i] = s
    schemes = [best_round_scheme(m, parts, j) for j in range(16)]
    ref = O.Index.build(recs, sigma, 16)
    want, dt = _timed(lambda: O.search_best(ref, reads, schemes, nthreads=ORACLE_THREADS))
    return dict(name="best16", sigma=sigma, edit=True, k=15, m=m, recs=recs, reads=reads, pats=reads, reverse=False,
                schemes=schemes, want=want, errs=set(range(16)), oracle_s=dt)


# ------------------------------------ e. the scheme table at its limits ----

TABLE = {"255x60": (255, 60), "240x64": (240, 64)}  # searches, m: 15300 and exactly 15360 entries


def filled_scheme(nsearch, m):
    """h2-k2's three Hamming k = 2 searches, repeated to nsearch searches."""
    pi, l, u = O.scheme("h2-k2", 0, 2, m, hamming=True)
    assert len(pi) == 3
    rep = lambda a: np.ascontiguousarray(np.tile(a, (-(-nsearch // 3), 1))[:nsearch])
    return rep(pi), rep(l), rep(u)


@functools.lru_cache(maxsize=None)
def table(name):
    """Duplicate searches multiply the multiset of rows on both sides alike."""
    nsearch, m = TABLE[name]
    rng = np.random.default_rng(nsearch * m)
    recs = random_records(rng, [3000, 1500], 6, with_n=True, repeats=True)
    reads = np.vstack([substituted_reads(rng, recs, 96, m, 2, 6), record_ends(recs, m)])
    return _search_case(name, 6, False, 2, recs, reads, filled_scheme(nsearch, m), range(3))


# --------------------------------------------------- f. long patterns ----

LONG = {  # name: (m, edit, k, sigma)
    "m4096-edit-k1": (4096, True, 1, 6),
    "m4096-hamming-k2": (4096, False, 2, 5),
    "m15360-edit-k1": (15360, True, 1, 5),
    "m15360-hamming-k2": (15360, False, 2, 6),
}
LONG_LENGTHS = [40000, 700, 90]
ALIGN_LONGEST = 16383  # sahara_gpu_align's longest pattern


@functools.lru_cache(maxsize=None)
def long_records(sigma):
    return random_records(np.random.default_rng(4000 + sigma), LONG_LENGTHS, sigma, with_n=True)


@functools.lru_cache(maxsize=None)
def long(name):
    """One search (backtracking): the long record's first and last m symbols
    and 14 reads from inside it, with 0 or 1 edits (Hamming: 0..2 substitutions)."""
    m, edit_, k, sigma = LONG[name]
    rng = np.random.default_rng(m + 10 * k + sigma)
    recs = long_records(sigma)
    body = edits_by_classes(rng, recs, 14, m, k, sigma) if edit_ else substituted_reads(rng, recs, 14, m, k, sigma)
    reads = np.vstack([recs[0][None, :m], recs[0][None, -m:], body])
    scheme = O.scheme("backtracking", 0, k, m, hamming=not edit_)
    assert len(scheme[0]) == 1
    return _search_case(name, sigma, edit_, k, recs, reads, scheme, range(k + 1))


@functools.lru_cache(maxsize=None)
def align_longest(sigma=6):
    """8 reads of 16383 symbols straight from the long record, read i with i
    substitutions (read 7: 8), at positions known by construction: (records,
    reads, (record, position) per read, substitutions per read)."""
    rng = np.random.default_rng(16383)
    recs = long_records(sigma)
    alpha = acgt(sigma)
    m = ALIGN_LONGEST
    starts = [0, len(recs[0]) - m] + [int(x) for x in rng.integers(1, len(recs[0]) - m, 6)]
    subs = [0, 1, 2, 3, 4, 5, 6, 8]
    reads = np.zeros((8, m), np.uint8)
    for i, (t, n) in enumerate(zip(starts, subs)):
        s = recs[0][t:t + m].copy()
        for j in rng.choice(m, size=n, replace=False):
            s[j] = rng.choice(alpha[alpha != s[j]])
        reads[i] = s
    return recs, reads, [(0, t) for t in starts], subs
