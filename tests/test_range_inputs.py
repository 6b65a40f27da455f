"""What each input of tests/range_cases.py exists for, asserted with the oracle
alone (no GPU): the error counts in its rows, a hit at position 0 of a record
and one that ends at a record's last symbol, the shape of its scheme, and the
oracle's wall time (printed; more than ORACLE_CAP_S fails). A case that stops
exercising its edge fails here, before tests/test_range_ends.py runs it."""
import numpy as np
import pytest

import oracle as O
import range_cases as R
import sahara_amd as sa
from helpers import hits_as_rows

MAX_ERRORS = 15  # the 4-bit fields (fm_layout.h packScheme, the compact hit records)


def _report(c):
    errs = sorted(set(c["want"][:, 3].tolist()))
    print(f'{c["name"]}: {len(c["want"])} rows, e {errs}, oracle {c["oracle_s"]:.2f} s')
    assert c["oracle_s"] <= R.ORACLE_CAP_S, (c["name"], c["oracle_s"])
    return errs


def _ref_lens(c):
    """Each row's record length."""
    return np.array([len(r) for r in c["recs"]], np.int64)[c["want"][:, 1].astype(np.int64)]


def _check(c):
    """Error counts exactly the case's own; record edges; every query a hit."""
    errs = _report(c)
    w = c["want"]
    assert set(errs) == c["errs"], (c["name"], errs)
    assert max(errs) <= MAX_ERRORS
    assert (w[:, 2] == 0).any(), "no hit at position 0 of a record"
    end = w[:, 2].astype(np.int64) + c["m"]
    assert (end >= _ref_lens(c)).any(), "no hit that reaches a record's last symbol"
    if not c["edit"]:
        assert (end <= _ref_lens(c)).all()  # (and none past it)
    return errs


@pytest.mark.parametrize("name", list(R.HAMMING))
def test_hamming_inputs(name):
    c = R.hamming(name)
    _check(c)
    gen, k, m, sigma, nsearch = R.HAMMING[name]
    assert c["reads"].shape == (100, m) and not c["reverse"]
    # read i carries i % (k + 1) substitutions, so its own position is a row of exactly that e
    per_q = {q: set() for q in range(96)}
    for q, _, _, e in c["want"][c["want"][:, 0] < 96].tolist():
        per_q[q].add(e)
    assert all(i % (k + 1) in per_q[i] for i in range(96))


def test_hamming_rc_input():
    c, plain = R.hamming("pigeon-k15", True), R.hamming("pigeon-k15")
    _check(c)
    assert c["reverse"] and c["pats"].shape == (200, 40)
    assert np.array_equal(c["pats"], sa.interleave_rc(c["reads"], c["sigma"]))  # the library's interleave, on the host
    assert np.array_equal(c["pats"][0::2], plain["pats"])
    fwd = c["want"][c["want"][:, 0] % 2 == 0].copy()
    fwd[:, 0] //= 2
    assert np.array_equal(fwd, plain["want"])


@pytest.mark.parametrize("name", list(R.EDIT))
def test_edit_inputs(name):
    c = R.edit(name)
    _check(c)
    gen, k, m, sigma, lengths, n = R.EDIT[name]
    assert 5 <= k <= 8 and c["reads"].shape == (n, m)
    per_q = np.bincount(c["want"][:, 0].astype(np.int64), minlength=n)
    print(f"  rows per query: max {per_q.max()}, queries with rows {np.count_nonzero(per_q)} of {n}")
    assert per_q.max() > 2048  # the sort's "huge" tier (locate_sort.hip), with e up to k in it
    assert np.array_equal(c["scheme"][0], sa.search_scheme(gen, 0, k, m)[0])


@pytest.mark.parametrize("name", list(R.STAIRCASE))
def test_staircase_inputs(name):
    c = R.staircase(name)
    errs = _check(c)
    m, parts, lag, sigma = R.STAIRCASE[name]
    pi, l, u = c["scheme"]
    assert pi.shape == (2, m) and u.max() == MAX_ERRORS and (l <= u).all()
    assert (np.diff(l.astype(np.int64), axis=1) >= 0).all() and (np.diff(u.astype(np.int64), axis=1) >= 0).all()
    assert np.array_equal(pi[0], np.arange(m)) and np.array_equal(pi[1], np.arange(m)[::-1])
    assert l[0, -1] == MAX_ERRORS - lag == min(errs)
    # both searches report: even reads by the first, odd reads by the second
    found = set(c["want"][:, 0].tolist())
    assert any(q % 2 == 0 for q in found) and any(q % 2 == 1 for q in found)
    for s in range(2):
        one = (pi[s:s + 1], l[s:s + 1], u[s:s + 1])
        rows = O.Index.build(c["recs"], sigma, 16).search(c["pats"], one, edit=True, nthreads=R.ORACLE_THREADS)[0]
        assert len(rows) and set((rows[:, 0] % 2).tolist()) == {s}, (s, len(rows))


def test_best16_input():
    c = R.best16()
    _check(c)
    assert len(c["schemes"]) == 16 and c["reads"].shape == (32, 96)
    for j, (pi, l, u) in enumerate(c["schemes"]):
        assert pi.shape == (1, 96) and u.max() == j == l[0, -1] and (l <= u).all()
    # every query is found, in the round of its own error count
    best = {}
    for q, _, _, e in c["want"].tolist():
        best.setdefault(q, set()).add(e)
    assert best == {q: {q // 2} for q in range(32)}
    # the reads from the stretch that stands in both records are found in both, with the same e
    both = {q for q in range(32) if {s for qq, s, _, _ in c["want"].tolist() if qq == q} == {0, 1}}
    assert both >= set(range(2, 32, 4)) and len(both) < 32  # (a read of record 1 may come from its copy as well)


@pytest.mark.parametrize("name", list(R.TABLE))
def test_table_inputs(name):
    c = R.table(name)
    _check(c)
    nsearch, m = R.TABLE[name]
    pi, l, u = c["scheme"]
    assert pi.shape == (nsearch, m) and nsearch <= 255 and nsearch * m <= 15360
    assert nsearch * m == {"255x60": 15300, "240x64": 15360}[name]
    # the same rows as the three searches alone, each nsearch / 3 times
    three = (pi[:3], l[:3], u[:3])
    once = O.Index.build(c["recs"], 6, 16).search(c["pats"], three, edit=False, nthreads=R.ORACLE_THREADS)[0]
    assert nsearch % 3 == 0 and len(c["want"]) == len(once) * (nsearch // 3)
    assert np.array_equal(np.unique(c["want"], axis=0), np.unique(hits_as_rows(once), axis=0))


@pytest.mark.parametrize("name", list(R.LONG))
def test_long_inputs(name):
    c = R.long(name)
    _check(c)
    m, edit, k, sigma = R.LONG[name]
    assert c["reads"].shape == (16, m) and c["scheme"][0].shape == (1, m)
    assert len(set(c["want"][:, 0].tolist())) == 16  # every read is found


def test_align_longest_input():
    recs, reads, places, subs = R.align_longest()
    assert reads.shape == (8, R.ALIGN_LONGEST) and max(subs) == 8 and min(subs) == 0
    assert places[0] == (0, 0) and places[1][1] + R.ALIGN_LONGEST == len(recs[0])
    for r, (s, t), n in zip(reads, places, subs):
        assert int((r != recs[s][t:t + R.ALIGN_LONGEST]).sum()) == n
