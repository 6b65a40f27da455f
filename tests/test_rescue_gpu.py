"""The mate rescue on the device (csrc/rescue.hip; docs/semantics.md "Mate
rescue") against tests/rescue_model.py: every call equals the pair rule over
the model's rescued rows, compared bit-exact as sorted rows, on the planted
case of tests/rescue_case.py: mates with 3 to 12 edits at the window's edges,
at a wave's round boundaries, in windows clipped by a record's ends, as equal
and unequal copies in one window, beside anchors with duplicates and
neighbours, and a tandem query that the anchor cap leaves alone."""
import functools

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows
from loci_model import loci
from pairs_case import K, M, SIGMA
from pairs_model import pairs
from rescue_case import CAP, KS, MAIN, SETTINGS, check, expect, model
from rescue_model import rescue
from test_golden import limit_rows

pytestmark = pytest.mark.gpu

OFF = dict(anchors=0, capped_queries=0, starts=0, rescued=0, batches=0, kernel_ms=0.0)
COUNTS = ("anchors", "capped_queries", "starts", "rescued")


def case():
    return check()  # (cached; asserts the case before any GPU call)


_GPU = {}


def gpu_of(device):
    if device not in _GPU:
        _GPU[device] = sa.BiFMIndex.build(case()["recs"], sigma=SIGMA, device=device)
    return _GPU[device]


class rescue_on:
    """set_pairs and set_rescue for a block, off again whatever happens in it."""

    def __init__(self, gpu, setting, Kr, A=0):
        self.gpu, self.args = gpu, (setting, Kr, A)

    def __enter__(self):
        setting, Kr, A = self.args
        self.gpu.set_pairs(*setting)
        self.gpu.set_rescue(Kr, A)
        return self.gpu

    def __exit__(self, *exc):
        self.gpu.set_rescue(None)
        self.gpu.set_pairs(None)
        self.gpu.set_loci(None)


def entry_points(gpu, c):
    pk = sa.pack_reads(c["reads"], SIGMA)
    yield "search", lambda: sa.search(gpu, c["pats"], c["scheme"])
    yield "search_reads", lambda: sa.search_reads(gpu, c["reads"], c["scheme"])
    yield "search_packed", lambda: sa.search_packed(gpu, pk, c["scheme"])
    yield "search_packed_compact", lambda: sa.search_packed_compact(gpu, pk, c["scheme"]).to_hits()

    def run_fetch():
        gpu.stage(c["pats"], c["scheme"])
        assert gpu.run() == gpu.stats()["hits"]
        return gpu.fetch()
    yield "run+fetch", run_fetch


def check_stats(gpu, counts, name):
    st = gpu.rescue_stats()
    for f in COUNTS:
        assert st[f] == counts[f], (name, f, st, counts)
    assert st["batches"] >= 1 and st["kernel_ms"] > 0, (name, st)


@pytest.mark.parametrize("batch", ["7", "260", None])
@pytest.mark.parametrize("Kr", KS)
def test_every_entry_point_returns_the_rescued_pairs(gpu_device, monkeypatch, Kr, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    want, counts = expect(MAIN, Kr), model(MAIN, Kr)[1]
    with rescue_on(gpu, MAIN, Kr):
        for name, call in entry_points(gpu, c):
            got = hits_as_rows(call())
            assert np.array_equal(got, want), (name, len(got), len(want))
            check_stats(gpu, counts, name)
            assert gpu.stats()["hits"] == len(want), name
            assert gpu.pairs_stats()["hits_in"] == len(c["want"]) + counts["rescued"], name
        # rescue off again, pairs still on: the pairs-only rows, and the stage's figures are zero
        gpu.set_rescue(None)
        for name, call in entry_points(gpu, c):
            assert np.array_equal(hits_as_rows(call()), pairs(c["want"], M, *MAIN)), name
            assert gpu.rescue_stats() == OFF, name
    assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), c["want"])


@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_windows_of_1_63_64_65_and_129_starts(gpu_device, setting):
    """A wave's round boundaries: the last start of a round, the first of the next, and a single start."""
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for Kr in KS:
        with rescue_on(gpu, setting, Kr):
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), expect(setting, Kr)), Kr
            check_stats(gpu, model(setting, Kr)[1], Kr)


@pytest.mark.parametrize("batch", ["7", None])
def test_the_anchor_cap_leaves_the_tandem_query_alone(gpu_device, monkeypatch, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    for Kr in (3, 8):
        want, counts = expect(MAIN, Kr, CAP), model(MAIN, Kr, CAP)[1]
        assert counts["capped_queries"] == 1 and len(want) < len(expect(MAIN, Kr))
        with rescue_on(gpu, MAIN, Kr, CAP):
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want), Kr
            check_stats(gpu, counts, Kr)
        with rescue_on(gpu, MAIN, Kr, 32):  # a cap the query stays under
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), expect(MAIN, Kr)), Kr
            check_stats(gpu, model(MAIN, Kr)[1], Kr)


@pytest.mark.parametrize("batch", ["7", "260"])
def test_with_loci_the_anchors_are_the_representatives(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    rep = loci(c["want"], 2)
    assert len(rep) < len(c["want"])
    pk = sa.pack_reads(c["reads"], SIGMA)
    for Kr in KS:
        want, counts = expect(MAIN, Kr, rows=rep, key="loci2"), model(MAIN, Kr, rows=rep, key="loci2")[1]
        assert counts["rescued"] > 0
        with rescue_on(gpu, MAIN, Kr):
            gpu.set_loci(2)
            for name, call in entry_points(gpu, c):
                assert np.array_equal(hits_as_rows(call()), want), (name, Kr)
                check_stats(gpu, counts, name)
                assert gpu.loci_stats()["loci"] == len(rep), name
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=1)), limit_rows(want, 1))


@pytest.mark.parametrize("batch", ["7", "260"])
@pytest.mark.parametrize("n", [1, 3])
def test_max_hits_runs_over_the_rescued_pairs(gpu_device, monkeypatch, n, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for Kr in KS:
        want = limit_rows(expect(MAIN, Kr), n)
        with rescue_on(gpu, MAIN, Kr):
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"], max_hits=n)), want)
            check_stats(gpu, model(MAIN, Kr)[1], "search")
            assert gpu.stats()["hits"] == len(want)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=n)), want)
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=n)), want)
    assert len(limit_rows(expect(MAIN, 8), 1)) < len(expect(MAIN, 8))


@functools.lru_cache(maxsize=None)
def best_case():
    c = case()
    schemes = [sa.search_scheme("h2-k2", j, j, M) for j in range(K + 1)]
    rows = hits_as_rows(O.search_best(c["ref"], c["pats"], schemes, nthreads=8))
    return schemes, rows


@pytest.mark.parametrize("batch", ["7", "260"])
def test_besthits_as_rounds_rescues_beside_the_stratum(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    schemes, rows = best_case()
    pk = sa.pack_reads(c["reads"], SIGMA)
    for Kr in KS:
        want, counts = expect(MAIN, Kr, rows=rows, key="best"), model(MAIN, Kr, rows=rows, key="best")[1]
        assert len(pairs(rows, M, *MAIN)) < len(want)
        with rescue_on(gpu, MAIN, Kr):
            for name, call in (("search_best", lambda: sa.search_best(gpu, c["pats"], schemes)),
                               ("search_best_reads", lambda: sa.search_best_reads(gpu, c["reads"], schemes)),
                               ("search_best_packed", lambda: sa.search_best_packed(gpu, pk, schemes)),
                               ("search_best_packed_compact",
                                lambda: sa.search_best_packed_compact(gpu, pk, schemes).to_hits())):
                assert np.array_equal(hits_as_rows(call()), want), (name, Kr)
                assert gpu.stats()["best_rounds"] == 3, name
                check_stats(gpu, counts, name)


def test_multi_part_index_rescues_per_part(gpu_device, monkeypatch):
    """The two records in two parts: each part's pass scans its own text."""
    c = case()
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "30500")
    gpu = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    monkeypatch.setenv("SAHARA_BATCH", "260")
    try:
        assert gpu.info()["n_parts"] == 2
        pk = sa.pack_reads(c["reads"], SIGMA)
        for Kr in KS:
            want, counts = expect(MAIN, Kr), model(MAIN, Kr)[1]
            gpu.set_pairs(*MAIN)
            gpu.set_rescue(Kr, 0)
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"])), want), Kr
            check_stats(gpu, counts, Kr)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want), Kr
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), want), Kr
            got = hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=3))
            assert np.array_equal(got, limit_rows(want, 3)), Kr
            gpu.stage(c["pats"], c["scheme"])
            assert gpu.run() == len(want)
            assert np.array_equal(hits_as_rows(gpu.fetch()), want), Kr
        # the cap counts a query's anchors per part: the tandem query's all lie in the first record's part
        for Kr in (3, 8):
            gpu.set_rescue(Kr, CAP)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), expect(MAIN, Kr, CAP)), Kr
            check_stats(gpu, model(MAIN, Kr, CAP)[1], Kr)
        gpu.set_rescue(None)
        assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"])), pairs(c["want"], M, *MAIN))
        assert gpu.rescue_stats() == OFF
    finally:
        gpu.close()


def test_hamming_scans_with_substitutions_only(gpu_device):
    """-d ham: the search and the scan both without indels."""
    c = case()
    gpu = gpu_of(gpu_device)
    scheme = sa.search_scheme("h2-k2", 0, K, M, hamming=True)
    rows = hits_as_rows(c["ref"].search(c["pats"], scheme, edit=False, nthreads=8)[0])
    for Kr in KS:
        st = {}
        want = pairs(rescue(rows, c["pats"], c["recs"], M, *MAIN, Kr, False, 0, st), M, *MAIN)
        assert st["rescued"] > 0 and len(want) < len(expect(MAIN, 8))
        with rescue_on(gpu, MAIN, Kr):
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], scheme, edit=False)), want), Kr
            check_stats(gpu, st, Kr)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], scheme, edit=False)), want), Kr


def test_overflow_rerun_gives_the_same_rows_and_stats(gpu_device, monkeypatch):
    """A hit buffer of 300 entries: the pipelined pass overflows and is redone
    serially; the stage's figures are those of the batches that count."""
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    gpu = gpu_of(gpu_device)
    with rescue_on(gpu, MAIN, 5):
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), expect(MAIN, 5))
        plain = gpu.rescue_stats()
    monkeypatch.setenv("SAHARA_HITCAP", "300")
    monkeypatch.setenv("SAHARA_TASKCAP", "200")
    small = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        small.set_pairs(*MAIN)
        small.set_rescue(5, 0)
        assert np.array_equal(hits_as_rows(sa.search_reads(small, c["reads"], c["scheme"])), expect(MAIN, 5))
        st = small.rescue_stats()
        assert small.stats()["pipelined"] == 0  # (the re-run is serial: the overflow happened)
        for f in COUNTS + ("batches",):
            assert st[f] == plain[f], (f, st, plain)
        assert st["kernel_ms"] > 0
    finally:
        small.close()


def test_call_time_refusals_leave_the_context_usable(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)

    def works():
        assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), expect(MAIN, 5))

    with rescue_on(gpu, MAIN, 5):
        works()
        gpu.set_pairs(None)  # rescue on, pairs off
        for call in (lambda: sa.search(gpu, c["pats"], c["scheme"]),
                     lambda: sa.search_reads(gpu, c["reads"], c["scheme"]),
                     lambda: sa.search_packed(gpu, pk, c["scheme"]),
                     lambda: sa.search_packed_compact(gpu, pk, c["scheme"]),
                     lambda: gpu.stage(c["pats"], c["scheme"]),
                     lambda: sa.search_best(gpu, c["pats"], best_case()[0])):
            with pytest.raises(sa.SaharaError, match="needs pairs on"):
                call()
        gpu.set_pairs(*MAIN)
        works()
        gpu.set_pairs(100, M + 52 + 4095)  # dmax - dmin = 4095: the widest window
        assert len(sa.search_packed(gpu, pk, c["scheme"])) > 0
        gpu.set_pairs(100, M + 52 + 4096)
        for call in (lambda: sa.search(gpu, c["pats"], c["scheme"]),
                     lambda: sa.search_packed(gpu, pk, c["scheme"]),
                     lambda: gpu.stage(c["pats"], c["scheme"])):
            with pytest.raises(sa.SaharaError, match="SAHARA_RESCUE_MAX_WINDOW"):
                call()
        gpu.set_pairs(*MAIN)
        works()
        # staged with rescue off, run with pairs off and rescue on
        gpu.set_rescue(None)
        gpu.stage(c["pats"], c["scheme"])
        gpu.set_pairs(None)
        gpu.set_rescue(5)
        with pytest.raises(sa.SaharaError, match="needs pairs on"):
            gpu.run()
        gpu.set_pairs(*MAIN)
        works()
        for bad in (0, 9):
            with pytest.raises(sa.SaharaError, match="max_err must be in"):
                gpu.set_rescue(bad)
            works()  # (the refused setting changed nothing)


def test_patterns_longer_than_the_alignment_takes_are_refused(gpu_device):
    """len = 16384, one above what the table's 16-bit entries hold: refused by
    every entry point before anything is staged, as the alignment calls refuse
    it; 16383 passes this check. (run() cannot meet such a length: no scheme
    of it can be staged, searches * len <= 15360.)"""
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    rng = np.random.default_rng(2)
    long = 16384
    reads = np.array([1, 2, 3, 5], np.uint8)[rng.integers(0, 4, size=(4, long))]
    pats = sa.interleave_rc(reads, SIGMA)
    lpk = sa.pack_reads(reads, SIGMA)
    pi = np.arange(long, dtype=np.uint32)[None, :]
    scheme = (pi, np.zeros_like(pi), np.zeros_like(pi))  # (never looked at: the length is refused first)
    with rescue_on(gpu, (0, long + 1000), 5):
        for name, call in (("search", lambda: sa.search(gpu, pats, scheme)),
                           ("search_reads", lambda: sa.search_reads(gpu, reads, scheme)),
                           ("search_packed", lambda: sa.search_packed(gpu, lpk, scheme)),
                           ("search_packed_compact", lambda: sa.search_packed_compact(gpu, lpk, scheme)),
                           ("stage", lambda: gpu.stage(pats, scheme)),
                           ("search_best", lambda: sa.search_best(gpu, pats, [scheme])),
                           ("search_best_reads", lambda: sa.search_best_reads(gpu, reads, [scheme])),
                           ("search_best_packed", lambda: sa.search_best_packed(gpu, lpk, [scheme])),
                           ("search_best_packed_compact", lambda: sa.search_best_packed_compact(gpu, lpk, [scheme]))):
            with pytest.raises(sa.SaharaError, match="is above 16383"):
                call()
            gpu.set_pairs(*MAIN)  # the context works on: the next call on it
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), expect(MAIN, 5)), name
            gpu.set_pairs(0, long + 1000)
        # one symbol fewer passes the rescue's check (and fails the next one: no scheme of that length is staged)
        short = pats[:, :long - 1]
        with pytest.raises(sa.SaharaError) as e:
            sa.search(gpu, short, tuple(x[:, :long - 1] for x in scheme))
        assert "is above 16383" not in str(e.value)


def test_alignment_of_the_rescued_hits_returns_their_err(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    with rescue_on(gpu, MAIN, 8):
        hits = sa.search(gpu, c["pats"], c["scheme"])
    rows = hits_as_rows(hits)
    assert np.array_equal(rows, expect(MAIN, 8))
    have = set(map(tuple, c["want"].tolist()))
    new = np.array([tuple(r) not in have for r in np.stack([hits["qid"], hits["seq_id"], hits["pos"], hits["err"]], 1).tolist()])
    assert new.sum() == model(MAIN, 8)[1]["rescued"]
    got = sa.align(gpu, c["pats"], hits[new], edit=True, max_err=8)
    assert np.array_equal(got["err"].astype(np.int64), hits[new]["err"].astype(np.int64))
    assert (hits[new]["err"] > K).all() and (hits[new]["err"] == 8).any()
