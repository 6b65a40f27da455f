"""The pair stage's links on the device (csrc/pairs.hip; docs/semantics.md
"Pair links") against tests/pair_links_model.py: every call's links equal the
model's on the oracle's rows, bit for bit, with the rows, the per-pair summary
and the figures, on the planted case of tests/best_pairs_case.py: ties,
non-mutual links, mates inside tandem runs whose ranges hold hundreds of rows
across blocks of 64 and workgroups."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
import rescue_case
from best_pairs_case import EXACT, K, M, SIGMA, WIDE
from best_pairs_model import stats_of
from helpers import hits_as_rows
from loci_model import loci
from pair_links_case import check, expected_links
from pair_links_model import LINK_DTYPE, PRIMARY, pair_links
from pairs_model import pair_count

pytestmark = pytest.mark.gpu

LINKS_OFF = dict(links=0, primaries=0, kernel_ms=0.0)
SETTINGS = (WIDE, EXACT)
DELTAS = (0, 1)


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


class links_on:
    """set_pairs, set_best_pairs and set_pair_links for a block on one of this
    module's contexts, which every test takes with all stages off: on leaving,
    whatever happened, every stage is off again."""

    def __init__(self, gpu, setting, delta):
        self.gpu, self.setting, self.delta = gpu, setting, delta

    def __enter__(self):
        self.gpu.set_pairs(*self.setting)
        self.gpu.set_best_pairs(self.delta)
        self.gpu.set_pair_links(True)
        return self.gpu

    def __exit__(self, *exc):
        self.gpu.set_pair_links(False)
        self.gpu.set_best_pairs(None)
        self.gpu.set_rescue(None)
        self.gpu.set_pairs(None)
        self.gpu.set_loci(None)


def entry_points(gpu, c, every=True):
    pk = sa.pack_reads(c["reads"], SIGMA)
    yield "search", lambda: sa.search(gpu, c["pats"], c["scheme"])
    yield "search_packed_compact", lambda: sa.search_packed_compact(gpu, pk, c["scheme"]).to_hits()
    if not every:
        return
    yield "search_reads", lambda: sa.search_reads(gpu, c["reads"], c["scheme"])
    yield "search_packed", lambda: sa.search_packed(gpu, pk, c["scheme"])

    def run_fetch():
        gpu.stage(c["pats"], c["scheme"])
        assert gpu.run() == gpu.stats()["hits"]
        return gpu.fetch()
    yield "run+fetch", run_fetch


def check_call(gpu, got, rows_in, model, name):
    """A call's rows, summary, links and figures against the model's."""
    kept, summary, links, info = model
    assert np.array_equal(hits_as_rows(got), kept), (name, len(got), len(kept))
    got_summary = gpu.pair_summary()
    assert got_summary.dtype == summary.dtype and np.array_equal(got_summary, summary), name
    got_links = gpu.pair_links()
    assert sa.PAIR_LINK_DTYPE == LINK_DTYPE and got_links.dtype == LINK_DTYPE and sa.LINK_PRIMARY == PRIMARY
    assert len(got_links) == len(links), (name, len(got_links), len(links))
    differ = np.flatnonzero(got_links != links)
    assert len(differ) == 0, (name, len(differ), differ[:5], got_links[differ[:5]], links[differ[:5]], kept[differ[:5]])
    # what the rule promises, on the device's own output
    at = np.arange(len(kept))
    there = at + got_links["mate"]
    prim = (got_links["flags"] & PRIMARY) != 0
    assert ((there >= 0) & (there < len(kept))).all(), name  # the mate of a kept record is kept
    assert (there[there[prim]] == at[prim]).all() and prim[there[prim]].all(), name
    pair = (kept[:, 0] >> np.uint64(2)).astype(np.int64)
    assert (got_links["score"][prim] == summary["best"][pair[prim]]).all(), name
    n_kept, n_pairs, n_unique = stats_of(kept, summary)
    ls = gpu.pair_links_stats()
    assert (ls["links"], ls["primaries"]) == (n_kept, 2 * n_pairs), (name, ls)
    st = gpu.best_pairs_stats()
    assert (st["hits_in"], st["kept"], st["pairs"], st["unique_pairs"]) == (len(rows_in), n_kept, n_pairs, n_unique), \
        (name, st)
    assert 0 < ls["kernel_ms"] < st["kernel_ms"], (name, ls, st)
    ps = gpu.pairs_stats()
    assert (ps["hits_in"], ps["kept"], ps["pairs"]) == (len(rows_in), n_kept, pair_count(kept)), (name, ps)


@pytest.mark.parametrize("batch", ["7", "260", None])
@pytest.mark.parametrize("delta", DELTAS)
def test_every_entry_point_returns_the_links(gpu_device, monkeypatch, delta, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    for setting in SETTINGS:
        model = expected_links(setting, delta)
        with links_on(gpu, setting, delta):
            every = (setting, delta, batch) == (WIDE, 0, "7")  # all five once; the whole-hit and the compact route always
            for name, call in entry_points(gpu, c, every):
                check_call(gpu, call(), c["want"], model, (name, setting))
                assert gpu.stats()["hits"] == len(model[0]), name


def test_links_do_not_change_the_call_and_off_again_it_is_what_it_was(gpu_device, monkeypatch):
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    gpu = gpu_of(gpu_device)
    kept, summary, links, info = expected_links(WIDE, 0)
    with links_on(gpu, WIDE, 0):
        check_call(gpu, sa.search(gpu, c["pats"], c["scheme"]), c["want"], expected_links(WIDE, 0), "on")
        gpu.set_pair_links(False)
        for name, call in entry_points(gpu, c):
            assert np.array_equal(hits_as_rows(call()), kept), name
            assert np.array_equal(gpu.pair_summary(), summary), name
            with pytest.raises(sa.SaharaError, match="without pair links"):
                gpu.pair_links()
            assert gpu.pair_links_stats() == LINKS_OFF, name
            st = gpu.best_pairs_stats()  # what tests/test_best_pairs_gpu.py expects of it
            assert (st["hits_in"], st["kept"], st["pairs"], st["unique_pairs"]) == \
                (len(c["want"]), *stats_of(kept, summary)), name
            assert st["batches"] >= 1 and st["kernel_ms"] > 0, name
    for name, call in entry_points(gpu, c):
        assert np.array_equal(hits_as_rows(call()), c["want"]), name
        assert gpu.pair_links_stats() == LINKS_OFF, name


@pytest.mark.parametrize("batch", ["7", "260"])
def test_with_loci_the_links_are_the_representatives(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    rep = loci(c["want"], 2)
    for setting, delta in ((WIDE, 0), (EXACT, 1)):
        model = pair_links(rep, M, *setting, delta, c["n_pairs"])
        assert len(model[0])
        with links_on(gpu, setting, delta):
            gpu.set_loci(2)
            for name, call in entry_points(gpu, c, every=False):
                check_call(gpu, call(), rep, model, (name, setting))


@pytest.mark.parametrize("batch", ["7", None])
def test_rescued_records_are_linked_like_any_others(gpu_device, monkeypatch, batch):
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
        gpu.set_pair_links(True)
        for delta in (0, 1):
            model = pair_links(rows, M, *rescue_case.MAIN, delta, len(c["reads"]) // 2)
            gpu.set_best_pairs(delta)
            for name, call in entry_points(gpu, c, every=False):
                check_call(gpu, call(), rows, model, (name, delta))
    finally:
        gpu.close()


@pytest.mark.parametrize("batch", ["7", "260"])
def test_besthits_as_rounds_the_links_are_the_stratums(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    schemes = [sa.search_scheme("h2-k2", j, j, M) for j in range(K + 1)]
    rows = hits_as_rows(O.search_best(c["ref"], c["pats"], schemes, nthreads=8))
    pk = sa.pack_reads(c["reads"], SIGMA)
    for delta in (0, 1):
        model = pair_links(rows, M, *WIDE, delta, c["n_pairs"])
        assert len(model[0])
        with links_on(gpu, WIDE, delta):
            for name, call in (("search_best", lambda: sa.search_best(gpu, c["pats"], schemes)),
                               ("search_best_packed_compact",
                                lambda: sa.search_best_packed_compact(gpu, pk, schemes).to_hits())):
                check_call(gpu, call(), rows, model, (name, delta))
                assert gpu.stats()["best_rounds"] == 3, name


def test_overflow_rerun_leaves_the_links_of_the_batches_that_count(gpu_device, monkeypatch):
    """A hit buffer of 300 entries: the pipelined pass overflows and is redone serially."""
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    monkeypatch.setenv("SAHARA_HITCAP", "300")
    monkeypatch.setenv("SAHARA_TASKCAP", "200")
    small = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        small.set_pairs(*WIDE)
        small.set_best_pairs(0)
        small.set_pair_links(True)
        check_call(small, sa.search_reads(small, c["reads"], c["scheme"]), c["want"], expected_links(WIDE, 0), "overflow")
        assert small.stats()["pipelined"] == 0  # (the re-run is serial: the overflow happened)
    finally:
        small.close()


def test_refusals_leave_the_context_usable(gpu_device, monkeypatch):
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    model = expected_links(WIDE, 1)

    def works():
        check_call(gpu, sa.search_packed(gpu, pk, c["scheme"]), c["want"], model, "works")

    calls = (lambda **kw: sa.search(gpu, c["pats"], c["scheme"], **kw),
             lambda **kw: sa.search_reads(gpu, c["reads"], c["scheme"], **kw),
             lambda **kw: sa.search_packed(gpu, pk, c["scheme"], **kw))
    with links_on(gpu, WIDE, 1):
        works()
        # links on, best pairs off
        gpu.set_best_pairs(None)
        for call in calls + (lambda: sa.search_packed_compact(gpu, pk, c["scheme"]),
                             lambda: gpu.stage(c["pats"], c["scheme"])):
            with pytest.raises(sa.SaharaError, match="pair links: needs best pairs on"):
                call()
        # staged with links off, run with them on and best pairs off
        gpu.set_pair_links(False)
        gpu.stage(c["pats"], c["scheme"])
        gpu.set_pair_links(True)
        with pytest.raises(sa.SaharaError, match="pair links: needs best pairs on"):
            gpu.run()
        gpu.set_best_pairs(1)
        works()
        # max_hits would cut linked records
        for call in calls:
            with pytest.raises(sa.SaharaError, match="pair links: a call with max_hits"):
                call(max_hits=3)
        works()
        # the links of a call that ran without them
        gpu.set_pair_links(False)
        sa.search_packed(gpu, pk, c["scheme"])
        gpu.set_pair_links(True)  # (the setting is of the next call)
        with pytest.raises(sa.SaharaError, match="without pair links"):
            gpu.pair_links()
        works()
    # a multi-part index: best pairs refuse it already
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "40500")
    parts = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    try:
        assert parts.info()["n_parts"] == 2
        parts.set_pairs(*WIDE)
        parts.set_best_pairs(0)
        parts.set_pair_links(True)
        with pytest.raises(sa.SaharaError, match="multi-part index"):
            sa.search(parts, c["pats"], c["scheme"])
    finally:
        parts.close()


def test_the_links_call_counts_and_checks_its_capacity(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    L = sa.lib()
    n = C.c_uint64(0)
    kept, summary, links, info = expected_links(WIDE, 0)
    with links_on(gpu, WIDE, 0):
        sa.search(gpu, c["pats"], c["scheme"])
        assert L.sahara_gpu_pair_links(gpu._h, None, 0, C.byref(n)) == 0 and n.value == len(links)  # the count alone
        out = np.zeros(len(links), sa.PAIR_LINK_DTYPE)
        assert L.sahara_gpu_pair_links(gpu._h, out.ctypes.data_as(C.c_void_p), len(links) - 1, C.byref(n)) < 0
        assert b"capacity too small" in L.sahara_gpu_last_error()
        assert L.sahara_gpu_pair_links(gpu._h, None, len(links), None) < 0
        assert b"null output" in L.sahara_gpu_last_error()
        assert L.sahara_gpu_pair_links(gpu._h, out.ctypes.data_as(C.c_void_p), len(links), None) == 0
        assert np.array_equal(out, links)
