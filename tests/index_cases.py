"""The case table of the index tests: texts at the sampling rates and the sizes
where index_build.hip's kernels and kLocate's LF walk change path.

One module-level list, CASES, shared by tests/test_index_model.py (oracle ==
model, no GPU) and tests/test_index_edges.py (device build, device load and
locate). records(), reference() and oracle_index() compute each case's inputs,
its model (tests/index_model.py) and the oracle's index once per process.
Every text has N <= 8193 symbols, delimiters included.
"""
import collections
import functools
import zlib

import numpy as np

from helpers import acgt, hits_as_rows, mutate_reads, random_records
from index_model import model

Case = collections.namedtuple("Case", "id kind sigma rate make")

RATE_LENS = [3000, 0, 1, 130, 1024, 63, 64, 65]
RATES = [1, 2, 3, 15, 16, 17, 32, 64, 100, 1000]
RATES_SIGMA5 = [1, 17, 1000]
# one record of N - 1 symbols: around kPackText's 32-symbol blocks, the 64-row
# Occ lines (an extra empty line when 64 | N; kLinesLocal's 16-byte-load path
# for base + 64 <= N), and kDensify's 16 rows per lane (the tail mask r16 + 16
# > N), 1024 per wave and 4096 per workgroup
SIZES = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049,
         4095, 4096, 4097, 8191, 8192, 8193]
SPLIT_SIZES = [64, 1024, 4096, 8192]
# prefix doubling sorts by 21 symbols, then by 42, 84, 168: an LCP on each step
LCPS = [20, 21, 22, 41, 42, 43, 83, 84, 85, 167, 168, 169]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rate_text(name, sigma):
    return random_records(_rng(name), RATE_LENS, sigma, with_n=True)


def _single(name, n):
    return random_records(_rng(name), [n - 1], 6)


def _split(name, n):
    """N symbols in records of 30-90: dense samples, a delimiter in most Occ lines."""
    rng = _rng(name)
    lens, left = [], n
    while left > 2 * 91:
        lens.append(int(rng.integers(30, 91)))
        left -= lens[-1] + 1
    lens.append(left // 2 - 1)  # two records take what is left (62..182 symbols, delimiters included)
    lens.append(left - lens[-1] - 2)
    assert sum(lens) + len(lens) == n and all(30 <= x <= 90 for x in lens), (n, lens)
    return random_records(rng, lens, 6)


def _planted(name, L, at_end):
    """A 2000-symbol record in which a segment of L symbols stands twice, with
    different symbols before and after the two copies: two suffixes with an LCP
    of exactly L. at_end: the second copy ends the last record, so the tie is
    broken by the delimiter and the end of the text."""
    rng = _rng(name)
    first = random_records(rng, [200], 6) if at_end else []
    r = random_records(rng, [2000], 6)[0]
    a = 300
    b = 2000 - L if at_end else 1200
    r[b:b + L] = r[a:a + L]
    r[a - 1], r[b - 1] = 1, 2          # before
    r[a + L] = 3                       # after the first copy
    if not at_end:
        r[b + L] = 5                   # after the second (at_end: the delimiter)
    return first + [r]


def _empty(name, where):
    recs = random_records(_rng(name), [120, 40, 77], 6)
    recs.insert({"first": 0, "middle": 2, "last": 3}[where], np.zeros(0, np.uint8))
    return recs


def _table():
    t = []
    for rate in RATES:
        t.append(Case(f"rate{rate}-s6", "rate", 6, rate, functools.partial(_rate_text, "rates-s6", 6)))
    for rate in RATES_SIGMA5:
        t.append(Case(f"rate{rate}-s5", "rate", 5, rate, functools.partial(_rate_text, "rates-s5", 5)))
    for n in SIZES:
        t.append(Case(f"n{n}", "size", 6, 16, functools.partial(_single, f"n{n}", n)))
    for n in SPLIT_SIZES:
        t.append(Case(f"n{n}-split", "size", 6, 16, functools.partial(_split, f"n{n}-split", n)))
    for L in LCPS:
        for at_end in (False, True):
            name = f"lcp{L}" + ("-end" if at_end else "")
            t.append(Case(name, "doubling", 6, 16, functools.partial(_planted, name, L, at_end)))
    t.append(Case("homopolymer", "doubling", 6, 16, lambda: [np.full(2047, 1, np.uint8)]))
    t.append(Case("poly-c-x5-rate3", "doubling", 6, 3, lambda: [np.full(100, 2, np.uint8) for _ in range(5)]))
    t.append(Case("period3-rate7", "doubling", 6, 7,
                  lambda: [np.resize(np.array([1, 2, 3], np.uint8), L) for L in (300, 301, 302, 64)]))
    t.append(Case("identical-x3", "doubling", 6, 16, lambda: [random_records(_rng("identical"), [500], 6)[0]] * 3))
    for where in ("first", "middle", "last"):
        name = f"empty-{where}"
        t.append(Case(name, "doubling", 6, 16, functools.partial(_empty, name, where)))
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the contexts that locate (LF walks and SA reads) is run on
LOCATE_CASES = [c for c in CASES if c.kind == "rate" or (c.kind == "size" and int(c.id[1:].split("-")[0]) >= 1023)]


@functools.lru_cache(maxsize=None)
def records(case_id):
    recs = [np.asarray(r, np.uint8) for r in BY_ID[case_id].make()]
    for r in recs:
        r.setflags(write=False)
    assert sum(len(r) + 1 for r in recs) <= 8193
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    c = BY_ID[case_id]
    return model(records(case_id), c.sigma, c.rate)


@functools.lru_cache(maxsize=None)
def oracle_index(case_id):
    import oracle as O
    c = BY_ID[case_id]
    return O.Index.build(list(records(case_id)), c.sigma, c.rate)


LOCATE_M, LOCATE_K = 24, 2


@functools.lru_cache(maxsize=None)
def locate_inputs(case_id):
    """(patterns, the oracle's sorted rows, its counters) of a locate case: 100
    reads of the text with up to two edits, searched with h2-k2. The patterns
    depend on the text alone, so the cases of one text at several rates locate
    the same rows and differ only in their LF walks."""
    import oracle as O
    c = BY_ID[case_id]
    recs = list(records(case_id))
    rng = np.random.default_rng(1000 * c.sigma + sum(len(r) + 1 for r in recs))
    pats = mutate_reads(rng, recs, 100, LOCATE_M, LOCATE_K, c.sigma)
    rows, cnt = oracle_index(case_id).search(pats, O.scheme("h2-k2", 0, LOCATE_K, LOCATE_M), edit=True)
    return pats, hits_as_rows(rows), cnt


def rate_offset(sigma, n_records):
    """Byte offset of the u64 sampling rate in a single-part .idx image: after
    sigma, the magic, n, C[0..sigma], the record count and the record lengths."""
    return 8 * (3 + sigma + 1 + 1 + n_records)


# ---- degenerate texts: records around the pattern length -------------------

DEGENERATE = [  # sigma, edit, m, k
    (6, True, 24, 2),
    (5, True, 30, 3),
    (6, False, 24, 2),
    (6, True, 24, 0),
]


# texts shorter than the pattern: (records, m, k, patterns)
_ACG_C = ([1, 2, 3], [2])
TINY = {
    # the N = 2 index: nothing of four symbols is within two edits of one symbol
    "n2-m4": (([1],), 4, 2, [[1, 1, 1, 1], [1, 2, 3, 5], [5, 1, 1, 2]]),
    # eight symbols against records of three and one: no hit, no error
    "acg-c-m8": (_ACG_C, 8, 2, [[1, 2, 3, 2, 1, 2, 3, 2], [1, 2, 3, 1, 2, 3, 1, 2], [2, 2, 2, 2, 2, 2, 2, 2]]),
    # ACGC against ACG$C$: five rows at record 0, position 0 (two with one error, three with two)
    "acg-c-m4": (_ACG_C, 4, 2, [[1, 2, 3, 2], [1, 2, 3, 5], [1, 2, 2, 3], [2, 2, 2, 2], [1, 1, 2, 3]]),
}


def tiny(name):
    recs, m, k, pats = TINY[name]
    return [np.array(r, np.uint8) for r in recs], m, k, np.array(pats, np.uint8)


@functools.lru_cache(maxsize=None)
def degenerate(sigma, edit, m, k):
    """(records, patterns): records of m-k-2 .. m+k+2 symbols and of 0, 1 and 2
    — shorter than, as long as and barely longer than the pattern, so the
    text-phase window is clamped at both ends at once — and patterns made of
    them: a record of m or more symbols cut to m from either end, a shorter
    one padded to m with random symbols at the front, at the back and at a
    random inside position. Every other pattern gets one substitution."""
    rng = _rng(f"degenerate-{sigma}-{edit}-{m}-{k}")
    lens = list(range(m - k - 2, m + k + 3)) + [0, 1, 2]
    recs = random_records(rng, lens, sigma)
    alpha = acgt(sigma)
    pats = []
    for r in recs:
        if len(r) >= m:
            pats += [r[:m], r[len(r) - m:]]
        else:
            pad = alpha[rng.integers(0, 4, size=m - len(r))]
            cut = int(rng.integers(0, len(r) + 1))
            pats += [np.concatenate([pad, r]), np.concatenate([r, pad]), np.concatenate([r[:cut], pad, r[cut:]])]
    pats = np.array(pats, np.uint8)
    for i in range(1, len(pats), 2):
        j = int(rng.integers(m))
        pats[i, j] = rng.choice(alpha[alpha != pats[i, j]])
    assert len(pats) <= 100
    return tuple(recs), pats
