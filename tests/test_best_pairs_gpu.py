"""The pair stage's best mode on the device (csrc/pairs.hip; docs/semantics.md
"Best pairs") against tests/best_pairs_model.py: every call equals the model
on the oracle's rows, compared bit-exact as sorted rows, with the per-pair
summary and the stage's figures, on the planted case of
tests/best_pairs_case.py: copies of a mate at different costs, ties, both
orientations, and mates inside tandem runs whose windows hold hundreds of
rows across blocks of 64 and workgroups."""
import functools

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
import rescue_case
from best_pairs_case import DELTAS, EXACT, K, M, SETTINGS, SIGMA, WIDE, check, expected
from best_pairs_model import best_pairs, stats_of
from helpers import hits_as_rows
from loci_model import loci
from pairs_model import pair_count, pairs
from test_golden import limit_rows

pytestmark = pytest.mark.gpu

OFF = dict(hits_in=0, kept=0, pairs=0, unique_pairs=0, batches=0, kernel_ms=0.0)
PAIRS_OFF = dict(hits_in=0, kept=0, pairs=0, batches=0, kernel_ms=0.0)


def case():
    return check()  # (cached; asserts the case before any GPU call)


_GPU = {}


def gpu_of(device):
    if device not in _GPU:
        _GPU[device] = sa.BiFMIndex.build(case()["recs"], sigma=SIGMA, device=device)
    return _GPU[device]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """The module's contexts (gpu_of) are its own and end with it."""
    yield
    while _GPU:
        _GPU.popitem()[1].close()


class best_on:
    """set_pairs and set_best_pairs for a block on one of this module's
    contexts (gpu_of), which every test takes with all stages off: on leaving,
    whatever happened, every stage is off again, those a test set inside the
    block (loci, rescue) included."""

    def __init__(self, gpu, setting, delta):
        self.gpu, self.setting, self.delta = gpu, setting, delta

    def __enter__(self):
        self.gpu.set_pairs(*self.setting)
        self.gpu.set_best_pairs(self.delta)
        return self.gpu

    def __exit__(self, *exc):
        self.gpu.set_best_pairs(None)
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


def same_summary(got, want):
    assert got.dtype == sa.PAIR_SUMMARY_DTYPE and got.dtype == want.dtype
    return np.array_equal(got, want)


def check_call(gpu, got, rows_in, kept, summary, name, left=None):
    """A call's rows, summary and figures against the model's; left: what --max_hits left of `kept`."""
    assert np.array_equal(hits_as_rows(got), kept if left is None else left), (name, len(got), len(kept))
    assert same_summary(gpu.pair_summary(), summary), name
    st = gpu.best_pairs_stats()
    n_kept, n_pairs, n_unique = stats_of(kept, summary)
    assert (st["hits_in"], st["kept"], st["pairs"], st["unique_pairs"]) == (len(rows_in), n_kept, n_pairs, n_unique), \
        (name, st)
    assert st["batches"] >= 1 and st["kernel_ms"] > 0, (name, st)
    # the pair stage's own figures: kept counts what leaves the stage
    ps = gpu.pairs_stats()
    assert (ps["hits_in"], ps["kept"], ps["pairs"]) == (len(rows_in), n_kept, pair_count(kept)), (name, ps)
    assert ps["batches"] == st["batches"] and ps["kernel_ms"] == st["kernel_ms"], name


@pytest.mark.parametrize("batch", ["7", "260", None])
@pytest.mark.parametrize("delta", DELTAS)
def test_every_entry_point_returns_the_best_pairs(gpu_device, monkeypatch, delta, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    for setting in SETTINGS:
        kept, summary = expected(setting, delta)
        with best_on(gpu, setting, delta):
            for name, call in entry_points(gpu, c):
                check_call(gpu, call(), c["want"], kept, summary, (name, setting))
                assert gpu.stats()["hits"] == len(kept), name


def test_off_again_every_call_is_what_it_was(gpu_device, monkeypatch):
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    gpu = gpu_of(gpu_device)
    paired = pairs(c["want"], M, *WIDE)
    with best_on(gpu, WIDE, 0):
        assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"])), expected(WIDE, 0)[0])
        gpu.set_best_pairs(None)
        for name, call in entry_points(gpu, c):
            assert np.array_equal(hits_as_rows(call()), paired), name
            assert gpu.best_pairs_stats() == OFF, name
            st = gpu.pairs_stats()  # what tests/test_pairs_gpu.py expects of it
            assert (st["hits_in"], st["kept"], st["pairs"]) == (len(c["want"]), len(paired), pair_count(paired)), name
            assert st["batches"] >= 1 and st["kernel_ms"] > 0, name
            with pytest.raises(sa.SaharaError, match="without best pairs"):
                gpu.pair_summary()
    for name, call in entry_points(gpu, c):
        assert np.array_equal(hits_as_rows(call()), c["want"]), name
        assert gpu.best_pairs_stats() == OFF and gpu.pairs_stats() == PAIRS_OFF, name


@pytest.mark.parametrize("batch", ["7", "260"])
@pytest.mark.parametrize("W", [0, 2])
def test_with_loci_the_rule_sees_the_representatives(gpu_device, monkeypatch, W, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    rep = loci(c["want"], W)
    for setting, delta in ((WIDE, 0), (EXACT, 1)):
        kept, summary = best_pairs(rep, M, *setting, delta, c["n_pairs"])
        assert 0 < len(kept) < len(pairs(rep, M, *setting)) or (setting == EXACT and len(kept))
        with best_on(gpu, setting, delta):
            gpu.set_loci(W)
            for name, call in entry_points(gpu, c):
                check_call(gpu, call(), rep, kept, summary, (name, setting, W))
                assert gpu.loci_stats()["loci"] == len(rep), name


@pytest.mark.parametrize("batch", ["7", "260"])
@pytest.mark.parametrize("n", [1, 3])
def test_max_hits_cuts_the_best_placements(gpu_device, monkeypatch, n, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for delta in (0, 30):
        kept, summary = expected(WIDE, delta)
        left = limit_rows(kept, n)
        assert len(left) < len(kept)
        with best_on(gpu, WIDE, delta):
            check_call(gpu, sa.search(gpu, c["pats"], c["scheme"], max_hits=n), c["want"], kept, summary, "search", left)
            assert gpu.stats()["hits"] == len(left)
            check_call(gpu, sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=n), c["want"], kept, summary,
                       "search_reads", left)
            check_call(gpu, sa.search_packed(gpu, pk, c["scheme"], max_hits=n), c["want"], kept, summary,
                       "search_packed", left)


@pytest.mark.parametrize("batch", ["7", None])
def test_rescued_records_compete_like_any_others(gpu_device, monkeypatch, batch):
    """tests/rescue_case.py's case: the mates the rescue finds join the hits before the rule runs."""
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = rescue_case.check()
    Kr = rescue_case.KS[1]
    rows = rescue_case.model(rescue_case.MAIN, Kr)[0]
    assert len(rows) > len(c["want"])
    gpu = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        gpu.set_pairs(*rescue_case.MAIN)
        gpu.set_rescue(Kr, 0)
        for delta in (0, 1):
            kept, summary = best_pairs(rows, M, *rescue_case.MAIN, delta, len(c["reads"]) // 2)
            plain = best_pairs(c["want"], M, *rescue_case.MAIN, delta, len(c["reads"]) // 2)[0]
            assert not np.array_equal(kept, plain)  # (the rescued records are among the best placements)
            gpu.set_best_pairs(delta)
            for name, call in entry_points(gpu, c):
                check_call(gpu, call(), rows, kept, summary, (name, delta))
    finally:
        gpu.close()


@pytest.mark.parametrize("batch", ["7", "260"])
def test_besthits_as_rounds_the_rule_sees_the_stratum(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    schemes = [sa.search_scheme("h2-k2", j, j, M) for j in range(K + 1)]
    rows = hits_as_rows(O.search_best(c["ref"], c["pats"], schemes, nthreads=8))
    pk = sa.pack_reads(c["reads"], SIGMA)
    for delta in (0, 1):
        kept, summary = best_pairs(rows, M, *WIDE, delta, c["n_pairs"])
        assert 0 < len(kept) < len(pairs(rows, M, *WIDE))
        with best_on(gpu, WIDE, delta):
            for name, call in (("search_best", lambda: sa.search_best(gpu, c["pats"], schemes)),
                               ("search_best_reads", lambda: sa.search_best_reads(gpu, c["reads"], schemes)),
                               ("search_best_packed", lambda: sa.search_best_packed(gpu, pk, schemes)),
                               ("search_best_packed_compact",
                                lambda: sa.search_best_packed_compact(gpu, pk, schemes).to_hits())):
                check_call(gpu, call(), rows, kept, summary, (name, delta))
                assert gpu.stats()["best_rounds"] == 3, name


def test_overflow_rerun_gives_the_same_rows_stats_and_summary(gpu_device, monkeypatch):
    """A hit buffer of 300 entries: the pipelined pass overflows and is redone
    serially; figures and summary are those of the batches that count."""
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    kept, summary = expected(WIDE, 0)
    monkeypatch.setenv("SAHARA_HITCAP", "300")
    monkeypatch.setenv("SAHARA_TASKCAP", "200")
    small = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        small.set_pairs(*WIDE)
        small.set_best_pairs(0)
        check_call(small, sa.search_reads(small, c["reads"], c["scheme"]), c["want"], kept, summary, "overflow")
        assert small.stats()["pipelined"] == 0  # (the re-run is serial: the overflow happened)
    finally:
        small.close()


def test_refusals_leave_the_context_usable(gpu_device, monkeypatch):
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    kept, summary = expected(WIDE, 1)

    def works():
        check_call(gpu, sa.search_packed(gpu, pk, c["scheme"]), c["want"], kept, summary, "works")

    with best_on(gpu, WIDE, 1):
        works()
        with pytest.raises(sa.SaharaError, match=r"delta must be in \[0, 30\]"):
            gpu.set_best_pairs(31)
        works()  # (the refused setting changed nothing)
        gpu.set_pairs(None)
        for call in (lambda: sa.search(gpu, c["pats"], c["scheme"]),
                     lambda: sa.search_reads(gpu, c["reads"], c["scheme"]),
                     lambda: sa.search_packed(gpu, pk, c["scheme"]),
                     lambda: sa.search_packed_compact(gpu, pk, c["scheme"]),
                     lambda: gpu.stage(c["pats"], c["scheme"])):
            with pytest.raises(sa.SaharaError, match="best pairs: needs pairs on"):
                call()
        # staged with the mode off, run with it on and pairs off
        gpu.set_best_pairs(None)
        gpu.stage(c["pats"], c["scheme"])
        gpu.set_best_pairs(1)
        with pytest.raises(sa.SaharaError, match="best pairs: needs pairs on"):
            gpu.run()
        gpu.set_pairs(*WIDE)
        works()
    # the two records in two parts
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "40500")
    parts = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    try:
        assert parts.info()["n_parts"] == 2
        parts.set_pairs(*WIDE)
        parts.set_best_pairs(0)
        for call in (lambda: sa.search(parts, c["pats"], c["scheme"]),
                     lambda: sa.search_reads(parts, c["reads"], c["scheme"]),
                     lambda: parts.stage(c["pats"], c["scheme"])):
            with pytest.raises(sa.SaharaError, match="multi-part index"):
                call()
        parts.set_best_pairs(None)
        assert np.array_equal(hits_as_rows(sa.search_reads(parts, c["reads"], c["scheme"])), pairs(c["want"], M, *WIDE))
        assert parts.best_pairs_stats() == OFF
    finally:
        parts.close()


def test_the_summary_call_counts_and_checks_its_capacity(gpu_device):
    import ctypes as C
    c = case()
    gpu = gpu_of(gpu_device)
    L = sa.lib()
    n = C.c_uint64(0)
    with best_on(gpu, WIDE, 0):
        sa.search(gpu, c["pats"], c["scheme"])
        assert L.sahara_gpu_pair_summary(gpu._h, None, 0, C.byref(n)) == 0 and n.value == c["n_pairs"]  # the count alone
        out = np.zeros(c["n_pairs"], sa.PAIR_SUMMARY_DTYPE)
        assert L.sahara_gpu_pair_summary(gpu._h, out.ctypes.data_as(C.c_void_p), c["n_pairs"] - 1, C.byref(n)) < 0
        assert b"capacity too small" in L.sahara_gpu_last_error()
        assert L.sahara_gpu_pair_summary(gpu._h, None, c["n_pairs"], None) < 0
        assert b"null output" in L.sahara_gpu_last_error()
        assert L.sahara_gpu_pair_summary(gpu._h, out.ctypes.data_as(C.c_void_p), c["n_pairs"], None) == 0
        assert np.array_equal(out, expected(WIDE, 0)[1])


def test_alignment_takes_the_kept_hits_as_any_hits(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    with best_on(gpu, EXACT, 0):
        hits = sa.search(gpu, c["pats"], c["scheme"])
    assert np.array_equal(hits_as_rows(hits), expected(EXACT, 0)[0])
    got = sa.align(gpu, c["pats"], hits, edit=True, max_err=K)
    assert len(got) == len(hits)
    assert (got["err"].astype(np.int64) <= K).all()
