"""The cases of tests/stage_caps_case.py proved without a GPU: what lets
tests/test_stage_caps_gpu.py take their tiled expectation as the truth and
run no oracle.

1. Every group type's rows by construction are the CPU oracle's rows for its
   four patterns, as search() takes them and as the packed entry points make
   them (with reverse complements): those and the random patterns find nothing.
2. Tiling equals the sequential models run on whole rows, for every stage
   combination the GPU file uses, on layouts of a couple of dozen groups.
3. Each big layout has the property it exists for: which rows lie on which
   side of row CAP = 8192 x 256, where a per-hit kernel's second trip starts."""
import functools

import numpy as np
import pytest

import oracle as O
import stage_caps_case as S
from helpers import hits_as_rows
from loci_model import loci
from pairs_model import pair_count, pairs
from rescue_model import rescue
from stage_caps_case import CAP, M, Stages
from test_golden import limit_rows

K0_LAYOUTS = (S.PAIRS_PARTIAL, S.PAIRS_ALL, S.PAIRS_NONE, S.PAIRS_MIXED, S.RESCUE, S.CHAIN)
K1_LAYOUTS = (S.LOCI,)


def _types(layouts):
    return sorted({typ for lay in layouts for typ in lay})


@functools.lru_cache(maxsize=None)
def _oracle():
    return O.Index.build(S.text().records, S.SIGMA, 16)


def _ham(k):
    return O.scheme("h2-k2", 0, k, M, hamming=True)


# ---- 1. the construction is the oracle's

@pytest.mark.parametrize("k,layouts", [(0, K0_LAYOUTS), (1, K1_LAYOUTS)], ids=["k0", "k1"])
def test_every_type_is_the_oracle_in_both_forms(k, layouts):
    types = _types(layouts)
    want = S.expected(types, k, Stages()).rows  # the types as one layout: group g is types[g]
    raw = S.patterns(types)
    packed = S.with_rc(S.reads(types))
    assert raw.shape == packed.shape == (4 * len(types), M)
    assert np.array_equal(raw[0::4], packed[0::4]) and np.array_equal(raw[3::4], packed[3::4])
    assert not np.array_equal(raw[1::4], packed[1::4])
    for name, pats in (("raw", raw), ("with reverse complements", packed)):
        got = hits_as_rows(_oracle().search(pats, _ham(k), edit=False, nthreads=8)[0])
        assert np.array_equal(got, want), name
        q = got[:, 0].astype(np.int64) % 4
        assert not ((q == 1) | (q == 2)).any(), name  # the random and the reverse-complement qids
        for g, typ in enumerate(types):
            for j in (0, 3):
                if typ[j] == 0:
                    assert not (got[:, 0] == 4 * g + j).any(), (name, typ)
    assert np.array_equal(np.bincount(want[:, 0].astype(np.int64) // 4, minlength=len(types)),
                          [len(S.group_rows(typ, k)) for typ in types])


def test_patterns_and_reads_of_a_layout():
    lay = [S.BIG, (3, 0, 0, 5), S.NONE, (0, 0, 0, 8), S.BIG]
    p, r = S.patterns(lay), S.reads(lay)
    t = S.text()
    assert np.array_equal(p[0], t.unit[4097]) and np.array_equal(p[3], t.unit[4096]) and np.array_equal(p[16:20], p[0:4])
    assert np.array_equal(p[11], t.random[3]) and np.array_equal(p[12], t.random[0])
    assert np.array_equal(S.with_rc(r)[3::4], p[3::4]) and np.array_equal(S.with_rc(r)[0::4], p[0::4])
    assert np.array_equal(S.rc(S.rc(p)), p)
    assert np.array_equal(S.rc(np.array([1, 2, 3, 5, 5], np.uint8)), [1, 1, 2, 3, 5])  # dna5: A C G T T -> A A C G T


# ---- 2. tiling equals the models on whole rows

def _mini(layout, extra=3):
    """Every type of the layout once, in its order there, and the first few groups again."""
    return list(dict.fromkeys(layout)) + list(layout[:extra])


def _whole(layout, k, st):
    """The models over all the layout's rows at once: (rows, figures)."""
    t = S.text()
    rows = t.expected([c for typ in layout for c in typ], k)
    fig = {}
    if st.W is not None:
        out = loci(rows, st.W)
        fig["loci"] = dict(hits_in=len(rows), loci=len(out))
        rows = out
    if st.rescue is not None:
        fig["rescue"] = {}
        rows = rescue(rows, S.patterns(layout), t.records, M, *st.frag, st.rescue[0], False, st.rescue[1], fig["rescue"])
    if st.frag is not None:
        out = pairs(rows, M, *st.frag)
        fig["pairs"] = dict(hits_in=len(rows), kept=len(out), pairs=pair_count(out))
        rows = out
    if st.limit and len(rows):
        rows = limit_rows(rows, st.limit)
    return rows, fig


COMBOS = ([(S.LOCI, 1, Stages(W=W, limit=n)) for W in S.LOCI_W for n in (0, 1, 3)]
          + [(S.PAIRS_PARTIAL, 0, Stages(frag=f)) for f in (S.NARROW, S.MIDDLE, S.WIDE)]
          + [(S.PAIRS_ALL, 0, Stages(frag=S.SELF)), (S.PAIRS_NONE, 0, Stages(frag=S.MIDDLE)),
             (S.PAIRS_MIXED, 0, Stages(frag=S.MIDDLE))]
          + [(S.RESCUE, 0, Stages(rescue=(Kr, A), frag=S.RESCUE_WINDOW)) for Kr in (1, 3) for A in (0, S.RESCUE_CAP)]
          + [(S.CHAIN, 0, S.CHAIN_STAGES)])


@pytest.mark.parametrize("layout,k,st", COMBOS, ids=[str(i) for i in range(len(COMBOS))])
def test_tiling_equals_the_models_on_whole_rows(layout, k, st):
    mini = _mini(layout)
    assert 8 <= len(mini) <= 40 and len(set(mini)) >= 7
    rows, fig = _whole(mini, k, st)
    e = S.expected(mini, k, st)
    assert np.array_equal(e.rows, rows)
    assert np.array_equal(hits_as_rows(e.rows), e.rows)  # canonical order as emitted
    assert e.figures == fig
    if st.rescue is not None:
        assert fig["rescue"]["rescued"] > 0


# ---- 3. what each case exists for

def _group_of(off, row):
    return int(np.searchsorted(off, row, side="right")) - 1


def test_quoted_figures_of_the_big_types():
    """300 groups of (4097, 0, 0, 4096) and 550 of (2048, 0, 0, 2048) alone."""
    for frag, kept in ((S.NARROW, 436_200), (S.MIDDLE, 1_357_800), (S.WIDE, 2_388_600)):
        e = S.expected([S.BIG] * 300, 0, Stages(frag=frag))
        assert e.figures["pairs"] == dict(hits_in=2_457_900, kept=kept, pairs=300) and len(e.rows) == kept
    for W, n, late in ((22, 2_112_000, 1100), (200, 948_200, None), (100000, 5_500, None)):
        tr = S.trace(S.TWINS, 1, Stages(W=W))
        assert 550 * tr.figures["loci"]["hits_in"] == 2_260_500 and 550 * tr.figures["loci"]["loci"] == n
        if late is not None:
            assert 550 * int(tr.mark["loci"]["late"].sum()) == late
    assert S.trace(S.TWINS, 1, Stages(W=100000)).mark["loci"]["sizes"].max() == 421
    for typ, finds in ((S.R64, 144), (S.R9, 61)):
        for Kr in (1, 3):
            tr = S.trace(typ, 0, Stages(rescue=(Kr, 0), frag=S.RESCUE_WINDOW))
            assert int(tr.mark["rescue"]["finds"].sum()) == finds
            assert 0 < tr.figures["rescue"]["rescued"] <= S.text().table[typ[3]][:, 2].sum()


def test_layouts_stay_in_one_batch_and_mix_their_types():
    for lay, k in [(lay, 0) for lay in K0_LAYOUTS] + [(S.LOCI, 1)]:
        assert 4 * len(lay) < 1 << 14  # far below a default batch of 2^21 patterns
        per = np.cumsum([0] + S.rows_of(lay, k))
        g = _group_of(per, CAP)
        assert per[g] < CAP < per[g + 1] - 1  # the seam is inside a group
        assert len(set(lay[max(0, g - 6):g + 7])) >= 2  # and not among blocks of one type
        # group boundaries at many offsets inside a wave
        assert len(set((per % 64).tolist())) >= 32, len(set((per % 64).tolist()))


@pytest.mark.parametrize("W", S.LOCI_W)
def test_loci_layout(W):
    st = Stages(W=W, limit=3)
    e = S.expected(S.LOCI, 1, st)
    assert e.entering["loci"] == e.figures["loci"]["hits_in"] > CAP
    rows, m, off = S.entering(S.LOCI, 1, st, "loci")
    sizes = np.concatenate([S.trace(typ, 1, st).mark["loci"]["sizes"] for typ in set(S.LOCI)])
    if W == 22:
        assert e.figures["loci"]["loci"] > CAP  # kLociGather's own second trip, and the limit stage's rows
        assert e.entering["limit"] > CAP
        assert m["head"][CAP]  # row CAP heads a locus
        assert m["late"][:CAP].any() and m["late"][CAP:].any()
    if W == 100000:
        assert not m["head"][CAP] and not m["head"][CAP - 1]  # rows CAP - 1 and CAP inside one locus
        assert sizes.max() >= 257 and (sizes >= 65).sum() >= 2
        assert e.figures["loci"]["loci"] < 10_000
    if W == 200:
        assert m["late"][:CAP].any() and m["late"][CAP:].any()
    # --max_hits: queries with more than 3 (so more than 1) representatives wholly on each side of the seam
    lrows, lm, loff = S.entering(S.LOCI, 1, st, "limit")
    seam = min(CAP, len(lrows) // 2)  # (the representatives pass CAP only at W = 22)
    g = _group_of(loff, seam)
    assert lm["cut"][:loff[g]].any() and lm["cut"][loff[g + 1]:].any()
    for n in (1, 3):
        assert len(S.expected(S.LOCI, 1, Stages(W=W, limit=n)).rows) < e.figures["loci"]["loci"]


def _seam_pairs(rows, keep):
    below, above = np.flatnonzero(keep[:CAP]), np.flatnonzero(keep[CAP:]) + CAP
    return int(below[-1]), int(above[0]), int(rows[below[-1], 0]) >> 2, int(rows[above[0], 0]) >> 2


@pytest.mark.parametrize("frag", [S.NARROW, S.MIDDLE, S.WIDE])
def test_pairs_partial_layout(frag):
    st = Stages(frag=frag)
    e = S.expected(S.PAIRS_PARTIAL, 0, st)
    assert e.entering["pairs"] > CAP and 0 < e.figures["pairs"]["kept"] < e.entering["pairs"]
    rows, m, off = S.entering(S.PAIRS_PARTIAL, 0, st, "pairs")
    keep = m["keep"]
    for side in (keep[:CAP], keep[CAP:]):
        assert side.any() and not side.all()
    lo, hi, p0, p1 = _seam_pairs(rows, keep)
    assert p0 == p1  # the kept record before the first kept one past the seam is of the same pair
    assert e.figures["pairs"]["pairs"] == len(np.unique(e.rows[:, 0] >> np.uint64(2)))


def test_pairs_all_and_none_layouts():
    e = S.expected(S.PAIRS_ALL, 0, Stages(frag=S.SELF))
    assert e.entering["pairs"] > CAP and e.figures["pairs"]["kept"] == e.entering["pairs"] == len(e.rows)
    assert e.figures["pairs"]["pairs"] == len(S.PAIRS_ALL)
    assert np.array_equal(e.rows, S.expected(S.PAIRS_ALL, 0, Stages()).rows)
    e = S.expected(S.PAIRS_NONE, 0, Stages(frag=S.MIDDLE))
    assert e.entering["pairs"] > CAP and len(e.rows) == 0
    assert e.figures["pairs"] == dict(hits_in=e.entering["pairs"], kept=0, pairs=0)


def test_pairs_mixed_layout():
    st = Stages(frag=S.MIDDLE)
    e = S.expected(S.PAIRS_MIXED, 0, st)
    assert e.entering["pairs"] > CAP + 100_000
    assert {S.BIG, S.ALL, S.NONE} <= set(S.PAIRS_MIXED)
    rows, m, off = S.entering(S.PAIRS_MIXED, 0, st, "pairs")
    keep = m["keep"]
    for side in (keep[:CAP], keep[CAP:]):
        assert side.any() and not side.all()
    lo, hi, p0, p1 = _seam_pairs(rows, keep)
    assert p0 != p1  # the kept record before the first kept one past the seam is of another pair,
    assert hi - lo > 4097 and not keep[lo + 1:hi].any()  # at least 4097 dropped rows back: 64 waves without a kept lane
    assert S.PAIRS_MIXED[_group_of(off, CAP)] == S.NONE
    # On both sides of the seam, kept rows whose wave holds no kept row before them (the 65 rows before are
    # dropped: such a row searches num for the kept record before it) and for which a search that reached
    # back only a wave or two would answer wrongly or by luck:
    #   own:   the dropped rows before it are its own pair's, the kept record before them another pair's
    #          (a search that ended among the dropped rows would not count the pair)
    #   other: the kept record before it is its own pair's, 1000 rows back or more
    at = np.flatnonzero(keep)
    gap = np.diff(at, prepend=-1)
    pair = (rows[:, 0] >> np.uint64(2)).astype(np.int64)
    far = at[gap > 65]
    far = far[far > 65]
    before = at[np.searchsorted(at, far) - 1]  # the kept record before each
    own = far[(pair[far - 65] == pair[far]) & (pair[before] != pair[far])]
    other = far[(pair[before] == pair[far]) & (far - before >= 1000)]
    for name, which in (("own", own), ("other", other)):
        assert (which < CAP).sum() >= 5 and (which >= CAP).sum() >= 5, (name, which)
    # the same layout cut for two batches: the first ends just past the seam
    lay, batch = S.two_batches(S.PAIRS_MIXED, 0)
    assert batch % 4 == 0 and len(lay) * 4 == 2 * batch
    per = np.cumsum([0] + S.rows_of(lay, 0))
    first, second = int(per[batch // 4]), int(per[-1] - per[batch // 4])
    assert CAP + 64 < first < CAP + 64 + 3 * 8194 and 0 < 50 * second < first
    k2 = S.entering(lay, 0, st, "pairs")[1]["keep"]
    assert k2[CAP:first].any() and not k2[CAP:first].all()


@pytest.mark.parametrize("Kr", [1, 3])
def test_rescue_layout(Kr):
    st = Stages(rescue=(Kr, 0), frag=S.RESCUE_WINDOW)
    e = S.expected(S.RESCUE, 0, st)
    f = e.figures["rescue"]
    assert e.entering["rescue"] > CAP and e.entering["pairs"] == e.entering["rescue"] + f["rescued"] > CAP
    assert 0 < f["rescued"] < f["anchors"] and f["capped_queries"] == 0
    assert 1_000_000 < f["anchors"] < e.entering["rescue"] and f["starts"] <= 4096 * f["anchors"]
    assert S.RESCUE_WINDOW[1] - M == 4095  # the widest window the stage takes
    rows, m, off = S.entering(S.RESCUE, 0, st, "rescue")
    g = _group_of(off, CAP)
    assert m["finds"][off[g + 1]:].any() and m["finds"][:off[g]].any()  # anchors wholly past the seam find their mate
    assert m["anchor"][CAP:].sum() > 10_000
    # the cap: the big queries are left alone, one of them across the seam; small ones are scanned on both sides
    sc = Stages(rescue=(Kr, S.RESCUE_CAP), frag=S.RESCUE_WINDOW)
    ec = S.expected(S.RESCUE, 0, sc)
    fc = ec.figures["rescue"]
    assert fc["capped_queries"] >= 2 * 360 and 0 < fc["rescued"] < fc["anchors"] < f["anchors"]
    assert len(ec.rows) < len(e.rows)
    q = int(rows[CAP, 0])
    assert int(rows[CAP - 1, 0]) == q  # row CAP is inside a query's segment,
    assert q % 4 in S.trace(S.RESCUE[q // 4], 0, sc).capped  # a capped one's
    small = [bool(S.trace(typ, 0, sc).uncapped) for typ in S.RESCUE]
    assert any(small[:g]) and any(small[g + 1:])
    for typ in set(S.RESCUE):
        tr = S.trace(typ, 0, sc)
        assert not set(tr.capped) & set(tr.uncapped)
        n = np.bincount(tr.rows_in["rescue"][tr.mark["rescue"]["anchor"], 0].astype(np.int64), minlength=4)
        assert n.max() <= S.RESCUE_CAP


def test_chain_layout():
    e = S.expected(S.CHAIN, 0, S.CHAIN_STAGES)
    for stage in ("loci", "rescue", "pairs", "limit"):
        assert e.entering[stage] > CAP, (stage, e.entering)
    f = e.figures
    assert f["loci"]["loci"] < f["loci"]["hits_in"] and 0 < f["rescue"]["rescued"] < f["rescue"]["anchors"]
    assert 0 < f["pairs"]["kept"] < f["pairs"]["hits_in"] == f["loci"]["loci"] + f["rescue"]["rescued"]
    assert 0 < len(e.rows) < f["pairs"]["kept"]
    for stage in ("rescue", "pairs", "limit"):
        rows, m, off = S.entering(S.CHAIN, 0, S.CHAIN_STAGES, stage)
        g = _group_of(off, CAP)
        assert off[g] < CAP < off[g + 1] - 1, stage  # the rewritten segments' seam is inside a group too
        if stage == "limit":
            assert m["cut"][:off[g]].any() and m["cut"][off[g + 1]:].any()
        if stage == "rescue":
            assert m["finds"][off[g + 1]:].any()
