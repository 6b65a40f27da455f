"""The post-sort stages (csrc/loci.hip, rescue.hip, pairs.hip, hits.hip
limitBatch / replaceBatch / kLociSegments) on batches of more than
CAP = 8192 x 256 rows: every per-hit kernel of these stages launches at most
8192 workgroups of 256 and walks the rest in a grid-stride loop, so past CAP a
thread makes a second trip, which is what the product does on every batch and
what no smaller case reaches.

The cases are tests/stage_caps_case.py's: groups of four queries over the
planted text, a few group types repeated hundreds of times in one batch, the
expectation tiled from the sequential models run once per type.
tests/test_stage_caps_case.py proves the construction equal to the CPU
oracle, the tiling equal to the models on whole rows, and each property named
below, all without a GPU; no oracle runs here. Every case asserts bit-exact
equality in canonical order (nothing is sorted, there is no tolerance) and the
stages' figures against the models' sums.

Seams, one line each (grep EDGE):

EDGE kLociHeads lane 0 reads h[i - 1] across the seam, row CAP inside a locus   test_loci[100000-0]
EDGE kLociHeads, row CAP heads a locus                                          test_loci[22-0]
EDGE kLociReduce, a locus of 421 rows across the seam meets in atomicMin        test_loci[100000-0]
EDGE kLociReduce, representatives that are not their locus's first row, both sides  test_loci[22-0], test_loci[200-0]
EDGE kLociGather past its own cap (2 112 000+ loci)                             test_loci[22-0]
EDGE kLociSegments over more than CAP representatives, read by limitBatch       test_loci[22-1], test_loci[22-3]
EDGE kPairFlags past the cap, three kept shares                                 test_pairs_partial
EDGE kPairGather's carried count and its lower bound into an earlier trip       test_pairs_partial, test_pairs_mixed
EDGE kPairGather, 4097+ dropped rows before the first kept row past the seam,
     the kept record before it of another pair                                  test_pairs_mixed
EDGE kPairGather, a wave's first kept row after hundreds of dropped rows of its
     own pair, or with its pair's kept record a thousand rows back, both sides  test_pairs_mixed
EDGE kPairGather with dst == nullptr (every record kept: j = i - 1)             test_pairs_all_kept
EDGE pairsBatch with nothing kept past the cap                                  test_pairs_none_kept
EDGE the seam next to a batch's end, a small batch after it                     test_pairs_mixed_two_batches
EDGE kRescueAnchorFlags reads h[i - 1] across the seam                          test_rescue
EDGE kRescueScan with anchors[blockIdx.x] above CAP, a million anchors          test_rescue[*-0]
EDGE kRescueCap, num[a - 1] and num[b - 1] of a query across the seam           test_rescue[*-100]
EDGE rescueMerge and replaceBatch over more than CAP records                    test_rescue, test_chain
EDGE kLociSegments after loci, after the rescue's merge and after pairs, each
     over more than CAP records that the next stage reads                       test_chain
EDGE limitBatch on more than CAP rows, queries cut on both sides                test_chain, test_loci[22-3]
"""
import functools

import numpy as np
import pytest

import sahara_amd as sa
import stage_caps_case as S
from stage_caps_case import CAP, M, SIGMA, Stages

pytestmark = pytest.mark.gpu

COUNTS = {"loci": ("hits_in", "loci"), "pairs": ("hits_in", "kept", "pairs"),
          "rescue": ("anchors", "capped_queries", "starts", "rescued")}


def _ham(k):
    return sa.search_scheme("h2-k2", 0, k, M, hamming=True)


def _same(h, want, what):
    """HIT_DTYPE array h == (n, 4) canonical rows, in order; the message names
    the first row that differs and where it lies from the seam."""
    cols = (h["qid"], h["seq_id"], h["pos"], h["err"])
    if len(h) == len(want) and all(np.array_equal(c, want[:, i]) for i, c in enumerate(cols)):
        return
    n = min(len(h), len(want))
    bad = np.zeros(n, bool)
    for i, c in enumerate(cols):
        bad |= c[:n] != want[:n, i]
    at = int(np.flatnonzero(bad)[0]) if bad.any() else n
    msg = (f"{what}: {len(h)} rows, expected {len(want)}; {int(bad.sum())} of the first {n} differ, "
           f"first at row {at} (CAP {at - CAP:+d})")
    if at < n:
        msg += f": got {tuple(int(c[at]) for c in cols)}, expected {tuple(int(x) for x in want[at])}"
    raise AssertionError(msg)


@pytest.fixture(scope="module")
def gpu(gpu_device):
    g = sa.BiFMIndex.build(S.text().records, sigma=SIGMA, device=gpu_device)
    yield g
    g.close()


class stages_on:
    """The stages' settings for a block, all off again whatever happens in it."""

    def __init__(self, gpu, st):
        self.gpu, self.st = gpu, st

    def __enter__(self):
        st = self.st
        if st.W is not None:
            self.gpu.set_loci(st.W)
        if st.frag is not None:
            self.gpu.set_pairs(*st.frag)
        if st.rescue is not None:
            self.gpu.set_rescue(*st.rescue)
        return self.gpu

    def __exit__(self, *exc):
        self.gpu.set_rescue(None)
        self.gpu.set_pairs(None)
        self.gpu.set_loci(None)


@functools.lru_cache(maxsize=4)
def _expected(name, k, st):
    return S.expected(getattr(S, name), k, st)


def _figures(gpu, e, what, batches=1):
    got = {"loci": gpu.loci_stats(), "pairs": gpu.pairs_stats(), "rescue": gpu.rescue_stats()}
    for stage, names in COUNTS.items():
        want = e.figures.get(stage, dict.fromkeys(names, 0))  # (a stage that is off reports zeros)
        assert {f: got[stage][f] for f in names} == want, (what, stage, got[stage])
        if stage in e.figures and e.entering[stage]:
            assert got[stage]["batches"] >= 1, (what, stage, got[stage])
    st = gpu.stats()
    assert st["hits"] == len(e.rows) and st["batches"] == batches, (what, st["hits"], st["batches"])


def _case(gpu, layout, e, k, st, fetch=False, batches=1):
    """The layout through search() on its patterns and through the packed
    entry point on its reads (compact records; with --max_hits, which the
    compact call does not take, whole hits), and through stage/run/fetch."""
    sch = _ham(k)
    pats = S.patterns(layout)
    pk = sa.pack_reads(S.reads(layout), SIGMA)
    assert pk.n_reads * 2 == len(pats) == 4 * len(layout)
    with stages_on(gpu, st):
        _same(sa.search(gpu, pats, sch, edit=False, max_hits=st.limit), e.rows, "search")
        _figures(gpu, e, "search", batches)
        if st.limit:
            _same(sa.search_packed(gpu, pk, sch, edit=False, max_hits=st.limit), e.rows, "search_packed")
            _figures(gpu, e, "search_packed", batches)
        else:
            c = sa.search_packed_compact(gpu, pk, sch, edit=False)
            try:
                _same(c.to_hits(), e.rows, "search_packed_compact")
            finally:
                c.close()
            _figures(gpu, e, "search_packed_compact", batches)
        if fetch:
            gpu.stage(pats, sch, edit=False)
            assert gpu.run() == len(e.rows)
            _same(gpu.fetch(), e.rows, "stage/run/fetch")
            _figures(gpu, e, "stage/run/fetch", batches)


# ---- loci, k = 1

@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("W", S.LOCI_W)
def test_loci(gpu, monkeypatch, W, n):
    """2 263 100 rows of 598 groups, 550 of them (2048, 0, 0, 2048): 2055 rows
    per query, 7 of them with e = 1. W = 22: more than CAP loci, row CAP heads
    one; W = 100000: one locus per record and query, 421 rows at most, rows
    CAP - 1 and CAP in one; then --max_hits n over the representatives."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(W=W, limit=n)
    e = _expected("LOCI", 1, st)
    assert e.entering["loci"] > CAP
    _case(gpu, S.LOCI, e, 1, st)


# ---- pairs, k = 0

@pytest.mark.parametrize("frag", [S.NARROW, S.MIDDLE, S.WIDE], ids=["narrow", "middle", "wide"])
def test_pairs_partial(gpu, monkeypatch, frag):
    """372 groups, 300 of them (4097, 0, 0, 4096): 8193 rows of which the
    window keeps 1454, 4526 or 7962."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(frag=frag)
    e = _expected("PAIRS_PARTIAL", 0, st)
    assert e.entering["pairs"] > CAP and 0 < len(e.rows) < e.entering["pairs"]
    _case(gpu, S.PAIRS_PARTIAL, e, 0, st)


def test_pairs_all_kept(gpu, monkeypatch):
    """Forward and reverse mate are one unit and min_fragment = 0,
    max_fragment = len: every row is its own partner's mate at distance 0."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(frag=S.SELF)
    e = _expected("PAIRS_ALL", 0, st)
    assert len(e.rows) == e.entering["pairs"] > CAP
    _case(gpu, S.PAIRS_ALL, e, 0, st)


def test_pairs_none_kept(gpu, monkeypatch):
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(frag=S.MIDDLE)
    e = _expected("PAIRS_NONE", 0, st)
    assert len(e.rows) == 0 and e.entering["pairs"] > CAP
    assert e.figures["pairs"]["kept"] == e.figures["pairs"]["pairs"] == 0
    _case(gpu, S.PAIRS_NONE, e, 0, st, fetch=True)


def test_pairs_mixed(gpu, monkeypatch):
    """Groups that keep a share, all, a handful and none of their rows in one
    batch of 2 678 897 rows; a group that keeps none lies across the seam."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(frag=S.MIDDLE)
    e = _expected("PAIRS_MIXED", 0, st)
    assert e.entering["pairs"] > CAP
    _case(gpu, S.PAIRS_MIXED, e, 0, st, fetch=True)


def test_pairs_mixed_two_batches(gpu, monkeypatch):
    """The mixed layout up to just past the seam, then as many small groups:
    with SAHARA_BATCH at half the patterns the first batch ends a few thousand
    rows past CAP and the second has a hundredth of its rows."""
    layout, batch = S.two_batches(S.PAIRS_MIXED, 0)
    monkeypatch.setenv("SAHARA_BATCH", str(batch))
    st = Stages(frag=S.MIDDLE)
    e = S.expected(layout, 0, st)
    _case(gpu, layout, e, 0, st, fetch=True, batches=2)


# ---- mate rescue, Hamming, search k = 0

@pytest.mark.parametrize("A", [0, S.RESCUE_CAP])
@pytest.mark.parametrize("Kr", [1, 3])
def test_rescue(gpu, monkeypatch, Kr, A):
    """762 groups, 360 each of (4097, 0, 0, 64) and (2049, 0, 0, 9), in the
    widest window (4096 starts): 1.56 million anchors, of which 205 per pair of
    such groups find a copy of the partner with one substitution. With the cap
    the big queries are left alone and the small groups' anchors are scanned."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    st = Stages(rescue=(Kr, A), frag=S.RESCUE_WINDOW)
    e = _expected("RESCUE", 0, st)
    assert e.entering["rescue"] > CAP and e.figures["rescue"]["rescued"] > 0
    assert (e.figures["rescue"]["capped_queries"] > 0) == (A > 0)
    _case(gpu, S.RESCUE, e, 0, st)


# ---- the chain

def test_chain(gpu, monkeypatch):
    """Loci at W = 22, the rescue, pairs and --max_hits 3 in one call: each
    stage is given more than CAP records, through segments the stage before
    it rewrote."""
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    e = _expected("CHAIN", 0, S.CHAIN_STAGES)
    assert all(e.entering[s] > CAP for s in ("loci", "rescue", "pairs", "limit"))
    _case(gpu, S.CHAIN, e, 0, S.CHAIN_STAGES)
    # without the cut, as compact records and through stage/run/fetch
    st = S.CHAIN_STAGES._replace(limit=0)
    _case(gpu, S.CHAIN, _expected("CHAIN", 0, st), 0, st, fetch=True)
