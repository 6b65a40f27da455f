"""The chain between the search kernels and the caller's buffer (locate_sort.hip, hits.hip
kTileSums .. kCompactHits), held at exact tier edges and past each grid cap.

The text is tests/planted.py's: the rows of every query are known by
construction (proved equal to the oracle's in tests/test_planted_model.py,
without a GPU), so a case of a million queries or 4.5M hits needs no oracle
run. Every case asserts bit-exact equality with that expectation, in the
canonical order the calls document: nothing is sorted here, and there is no
tolerance. The layouts are planted.py's data; their properties ("this range
sums to exactly 1024 rows") are asserted there.

Edges, one case each (grep EDGE):

EDGE tier 8|9, 64|65, skipped row, range of 1024 rows (tile path)  test_a_tier_edges[edges_1024 in LAYOUT_A]
EDGE range of 1025 rows (global path, same tiers)                  test_a_tier_edges[edges_1025 in LAYOUT_A]
EDGE 256 x 4, 1024 alone, 16 x 64, 64 medium lanes, zeros range    test_a_tier_edges[LAYOUT_A ranges]
EDGE record starts past the LDS table (300 records), dna4          test_a_tier_edges[300 records], [dna4]
EDGE long 65..2048 (P = n = 2048), huge 2049.., first/last/boundary test_b_long_and_huge_edges
EDGE nq 1, 255, 256, 257, 4095, 4096, 4097, twice per context      test_c_query_count_edges
EDGE ranges aligned and not aligned with batches (256, 257, 100)   test_c_batches_against_ranges
EDGE kScanPartials' second trip (> 1 048 576 patterns, one batch)  test_d_scan_carry
EDGE kSortBigLds past 4096 workgroups, lengths 65 and 2048         test_e_more_long_segments_than_workgroups
EDGE llist full: 4096 long queries in one scan tile                test_e_llist_full
EDGE kOffsetSeq past 8192 x 256 hits of one part, kQidKeys, kGatherHits test_e_5m_hits_three_parts
EDGE kExpandRecs (lazy), kDigest past 8192 x 256 hits               test_e_2m_hits_compact_fetch_digest
EDGE kCopyHits past 16384 x 256 hits, qid_offset                    test_e_4m_hits_copy
EDGE kDigest against bench.hits_digest                              test_f_digest
EDGE part merge, endBit at nq 1, 2, 3, 4, 5, 1024, 1025             test_g_part_merge
EDGE edit mode: keys that differ in e only, every tier             test_h_edit_mode
EDGE --max_hits quota at n = c0 - 1 .. c0 + c1 + 1                  test_max_hits_quota_edges
"""
import os
import sys

import numpy as np
import pytest

import oracle as O
import planted as P
import sahara_amd as sa
from helpers import hits_as_rows
from test_golden import limit_rows

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (read-only: hits_digest)

pytestmark = pytest.mark.gpu

MODES = ((True, True), (True, False), (False, True), (False, False))  # (verify, locate_sa)


def _ham(k):
    return sa.search_scheme("h2-k2", 0, k, P.M, hamming=True)


def _same(h, want, what, layout=None):
    """HIT_DTYPE array h == (n, 4) canonical rows, in order; the message names the first row that differs."""
    cols = (h["qid"], h["seq_id"], h["pos"], h["err"])
    if len(h) == len(want) and all(np.array_equal(c, want[:, i]) for i, c in enumerate(cols)):
        return
    n = min(len(h), len(want))
    bad = np.zeros(n, bool)
    for i, c in enumerate(cols):
        bad |= c[:n] != want[:n, i]
    at = int(np.flatnonzero(bad)[0]) if bad.any() else n
    msg = f"{what}: {len(h)} rows, expected {len(want)}; {int(bad.sum())} of the first {n} differ, first at row {at}"
    if at < n:
        q = int(want[at, 0])
        msg += f": got {tuple(int(c[at]) for c in cols)}, expected {tuple(int(x) for x in want[at])}"
        if layout is not None and q < len(layout):
            msg += f" (query {q}: {int(layout[q])} rows, {P.tier(int(layout[q]))})"
    raise AssertionError(msg)


def _routes(gpu, t, layout, want, sch, edit=False, compact=True):
    """The case through every route of a call's hits to the caller (a multi-part
    index has no compact calls: compact=False)."""
    pats = t.patterns(layout)
    if edit:  # the rows per query are the expectation's, not the layout's numbers
        layout = np.bincount(want[:, 0].astype(np.int64), minlength=len(pats))
    try:
        for verify, locate_sa in MODES:
            gpu.set_mode(verify=verify, locate_sa=locate_sa)
            _same(sa.search(gpu, pats, sch, edit=edit), want, f"search verify={verify} locate_sa={locate_sa}", layout)
    finally:
        gpu.set_mode(verify=True, locate_sa=True)
    _same(sa.search_reads(gpu, pats, sch, edit=edit, reverse=False), want, "search_reads", layout)
    if compact:
        c = sa.search_reads_compact(gpu, pats, sch, edit=edit, reverse=False)
        _same(c.to_hits(), want, "search_reads_compact", layout)
        c.close()
        c = sa.search_packed_compact(gpu, sa.pack_reads(pats, t.sigma, pinned=True), sch, edit=edit, reverse=False)
        _same(c.to_hits(), want, "search_packed_compact", layout)
        c.close()
    gpu.stage(pats, sch, edit=edit)
    assert gpu.run() == len(want)
    _same(gpu.fetch(), want, "stage/run/fetch", layout)


@pytest.fixture(scope="module")
def texts(gpu_device):
    """(planted text, context) per (sigma, records), built once: the cases
    share the contexts, as a caller's calls share one."""
    made = {}

    def get(sigma=6, nrec=5):
        if (sigma, nrec) not in made:
            t = P.build(sigma, nrec)
            made[sigma, nrec] = (t, sa.BiFMIndex.build(t.records, sigma=sigma, device=gpu_device))
        return made[sigma, nrec]
    yield get
    for _, g in made.values():
        g.close()


@pytest.fixture(scope="module")
def three_parts(gpu_device):
    """The 5-record text as an index of three parts."""
    t = P.build(6, 5)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SAHARA_PART_SYMBOLS", str(P.PART_SYMBOLS))
        gpu = sa.BiFMIndex.build(t.records, sigma=6, device=gpu_device)
    assert gpu.info()["n_parts"] == 3
    yield t, gpu
    gpu.close()


# ---- a. every tier edge, tile path and global path

@pytest.mark.parametrize("sigma,nrec", [(6, 5), (6, 300), (5, 5)], ids=["5 records", "300 records", "dna4"])
def test_a_tier_edges(texts, sigma, nrec):
    t, gpu = texts(sigma, nrec)
    _routes(gpu, t, P.LAYOUT_A, t.expected(P.LAYOUT_A, 0), _ham(0))


# ---- b. long and huge edges

@pytest.mark.parametrize("name", ["B1", "B2"])
@pytest.mark.parametrize("nrec", [5, 300])
def test_b_long_and_huge_edges(texts, nrec, name):
    t, gpu = texts(6, nrec)
    layout = getattr(P, "LAYOUT_" + name)
    _routes(gpu, t, layout, t.expected(layout, 0), _ham(0))


# ---- c. counts and batch edges

@pytest.mark.parametrize("nq", P.NQ_EDGES)
def test_c_query_count_edges(texts, nq):
    """Twice on the same context: kScanTiles zeroes the counts for the next batch."""
    t, gpu = texts()
    layout = P.layout_c(nq)
    want = t.expected(layout, 0)
    for _ in range(2):
        _routes(gpu, t, layout, want, _ham(0))


@pytest.mark.parametrize("batch", ["256", "257", "100"])
def test_c_batches_against_ranges(texts, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    t, gpu = texts()
    want = t.expected(P.LAYOUT_A, 0)
    for _ in range(2):
        _routes(gpu, t, P.LAYOUT_A, want, _ham(0))
    _same(sa.search(gpu, t.patterns(P.LAYOUT_A), _ham(0), edit=False), want, "search", P.LAYOUT_A)
    assert gpu.stats()["batches"] == -(-len(P.LAYOUT_A) // int(batch))


# ---- d. more than 1 048 576 patterns in one batch

def test_d_scan_carry(texts, monkeypatch):
    """kScanPartials' second trip: 257 scan tiles in one batch. The offsets of
    the last tile, and the long and the huge query listed from it, use the
    carried sum of the first 256 tiles. (1 575 427 rows.)"""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    t, gpu = texts()
    layout = P.layout_d()
    pats = t.patterns(layout)
    want = t.expected(layout, 0)
    assert len(want) == 1_575_427
    sch = _ham(0)
    _same(sa.search(gpu, pats, sch, edit=False), want, "search", layout)
    assert gpu.stats()["batches"] == 1 and gpu.stats()["patterns"] == P.NQ_D
    c = sa.search_reads_compact(gpu, pats, sch, edit=False, reverse=False)
    assert gpu.stats()["batches"] == 1 and len(c.block_end) == 1
    _same(c.to_hits(), want, "search_reads_compact", layout)
    c.close()


# ---- e. grid caps

@pytest.mark.parametrize("name", ["E_65", "E_MIXED"])
def test_e_more_long_segments_than_workgroups(texts, monkeypatch, name):
    """More than 4096 long segments in one batch: kSortBigLds strides. E_65:
    4200 x 65 rows (273 000); E_MIXED: 4097 x 65 and 103 x 2048 (477 249), with
    2048s past query 4096 too, so that a workgroup's second trip sorts 2048
    rows after 65 and 65 after 2048."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    t, gpu = texts()
    layout = getattr(P, "LAYOUT_" + name)
    _routes(gpu, t, layout, t.expected(layout, 0), _ham(0))
    assert gpu.stats()["batches"] == 1


def test_e_llist_full(texts, monkeypatch):
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    t, gpu = texts()
    _routes(gpu, t, P.LAYOUT_E_LLIST, t.expected(P.LAYOUT_E_LLIST, 0), _ham(0))
    assert gpu.stats()["batches"] == 1


def test_e_5m_hits_three_parts(three_parts):
    """1300 x 4097 = 5 326 100 hits over three parts of 2 107 300, 2 141 100
    and 1 077 700: kOffsetSeq, launched per part over that part's hits,
    strides past its 8192 x 256 threads in two of them; kQidKeys and
    kGatherHits stride over the merged total."""
    t, gpu = three_parts
    layout = P.LAYOUT_E_PARTS
    per_part = P.hits_per_part(t, layout)
    assert list(per_part) == [2_107_300, 2_141_100, 1_077_700] and per_part.max() > P.CAP_8192
    want = t.expected(layout, 0)
    assert len(want) == 5_326_100
    _same(sa.search(gpu, t.patterns(layout), _ham(0), edit=False), want, "search, three parts", layout)
    h = gpu.fetch()
    _same(h, want, "fetch, three parts", layout)
    assert gpu.digest() == bench.hits_digest(h)


def test_e_2m_hits_compact_fetch_digest(texts):
    """The same hits as compact records: to_hits(), then fetch() (the lazy
    kExpandRecs, past 8192 x 256) and digest() (kDigest, likewise); record
    starts in LDS (5 records) and in global memory (300)."""
    for nrec in (5, 300):
        t, gpu = texts(6, nrec)
        want = t.expected(P.LAYOUT_E_2M, 0)
        c = sa.search_reads_compact(gpu, t.patterns(P.LAYOUT_E_2M), _ham(0), edit=False, reverse=False)
        _same(c.to_hits(), want, "to_hits", P.LAYOUT_E_2M)
        c.close()
        h = gpu.fetch()
        _same(h, want, "fetch after a compact call", P.LAYOUT_E_2M)
        assert gpu.digest() == bench.hits_digest(h)


def test_e_4m_hits_copy(texts, gpu_device):
    """1100 x 4097 = 4 506 700 hits into a torch buffer: kCopyHits strides past 16384 x 256."""
    import torch
    from sahara_amd.dist import hit_rows_from_records
    t, gpu = texts()
    want = t.expected(P.LAYOUT_E_4M, 0, qid0=1000)
    n = len(want)
    assert n == 4_506_700 > P.CAP_16384
    gpu.stage(t.patterns(P.LAYOUT_E_4M), _ham(0), edit=False)
    assert gpu.run() == n
    buf = torch.full((n + 3, 3), -1, dtype=torch.int64, device=f"cuda:{gpu_device}")
    assert gpu.copy_hits(buf.data_ptr(), buf.shape[0], qid_offset=1000) == n
    host = buf.cpu().numpy()
    assert (host[n:] == -1).all()
    assert np.array_equal(hit_rows_from_records(host[:n]), want)


# ---- f. digest

def test_f_digest(texts):
    """kDigest against its host restatement on layout (a) and on no hits
    (2.46M and 5.33M hits: test_e_2m_hits_compact_fetch_digest, test_e_5m_hits_three_parts)."""
    t, gpu = texts()
    h = sa.search(gpu, t.patterns(P.LAYOUT_A), _ham(0), edit=False)
    assert len(h) == sum(P.LAYOUT_A)
    f = gpu.fetch()
    assert np.array_equal(f, h)
    assert gpu.digest() == bench.hits_digest(f) != 0
    assert len(sa.search(gpu, t.patterns([0] * 300), _ham(0), edit=False)) == 0
    f = gpu.fetch()
    assert len(f) == 0 and gpu.digest() == bench.hits_digest(f) == 0


# ---- g. part merge

@pytest.mark.parametrize("nq", P.NQ_PARTS)
def test_g_part_merge(texts, three_parts, nq):
    t, one = texts()
    _, gpu = three_parts
    layout = P.layout_g(nq)
    want = t.expected(layout, 0)
    pats = t.patterns(layout)
    _same(sa.search(one, pats, _ham(0), edit=False), want, "one part", layout)
    _routes(gpu, t, layout, want, _ham(0), compact=False)


# ---- h. edit mode

def test_h_edit_mode(texts):
    """Layout (a) under edit distance, k = 1: a copy is found at its position
    with e = 0 and at neighbouring positions with e = 1, so segments hold keys
    that differ only in e and positions reached twice. The oracle's rows are
    the expectation (43 172 rows, 25 146 distinct positions); by them the
    layout's 2560 queries are 1008 zero, 130 small, 1398 medium, 22 long and 2
    huge (a unit planted 4 times has 16 rows, one planted 64 times 234)."""
    t, gpu = texts()
    sch = sa.search_scheme("h2-k2", 0, 1, P.M)
    pats = t.patterns(P.LAYOUT_A)
    want = hits_as_rows(O.Index.build(t.records, 6, 16).search(pats, sch, edit=True, nthreads=8)[0])
    per_q = np.bincount(want[:, 0].astype(np.int64), minlength=len(pats))
    tiers = {P.tier(int(n)) for n in per_q}
    assert {"small", "medium", "long", "huge"} <= tiers
    assert len(np.unique(want[:, :3], axis=0)) < len(want)  # one position at two error counts
    _routes(gpu, t, P.LAYOUT_A, want, sch, edit=True)


# ---- --max_hits at the quota edges

_LIMIT_N = sorted({n for _, _, n, _ in P.limit_cases()})
_LIMIT_LAYOUT = [3, 0, 8, 64, 9, 2048, 1, 65] * 2


@pytest.mark.parametrize("n", _LIMIT_N)
def test_max_hits_quota_edges(texts, monkeypatch, n):
    """Hamming k = 1; the queries of (c0, c1) = (3, 5), (8, 1), (64, 5),
    (2048, 7) exact and one-substitution copies meet n at c0 - 1 .. c0 + c1 + 1
    (planted.limit_cases names the branch of each)."""
    t, gpu = texts()
    full = t.expected(_LIMIT_LAYOUT, 1)
    want = limit_rows(full, n)
    named = [(c0, c1, b) for c0, c1, m, b in P.limit_cases() if m == n]
    assert named
    for c0, c1, branch in named:  # the expectation is in the branch of limitPlan the case is named for
        e = want[want[:, 0] == _LIMIT_LAYOUT.index(c0), 3]
        exact, subst = int((e == 0).sum()), int((e == 1).sum())
        if branch == "all kept":             # distinct <= n
            assert (exact, subst) == (c0, c1) and c0 + c1 <= n
        elif branch == "ends at level 0":    # cum + hist[0] == n: eStar 0, the quota is the whole level
            assert (exact, subst) == (c0, 0) and n == c0
        elif branch == "cut inside level 0":
            assert (exact, subst) == (n, 0) and n < c0
        else:                                # cut inside level 1: all of level 0 and n - c0 of level 1's c1
            assert (exact, subst) == (c0, n - c0) and 0 < n - c0 < c1
    pats = t.patterns(_LIMIT_LAYOUT)
    sch = _ham(1)
    for batch in (None, "7"):
        if batch:
            monkeypatch.setenv("SAHARA_BATCH", batch)
        else:
            monkeypatch.delenv("SAHARA_BATCH", raising=False)
        _same(sa.search(gpu, pats, sch, edit=False, max_hits=n), want, f"search max_hits={n} batch={batch}")
        _same(sa.search_reads(gpu, pats, sch, edit=False, reverse=False, max_hits=n), want,
              f"search_reads max_hits={n} batch={batch}")
