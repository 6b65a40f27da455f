"""The pair stage on the device (csrc/pairs.hip; docs/semantics.md "Pairs")
against tests/pairs_model.py: every call equals pairs(oracle rows), compared
bit-exact as sorted rows, on the planted case of tests/pairs_case.py: pairs at
the window's edges, on two records, in the wrong order and orientation, with
copies of a mate inside and outside the window, and mates inside tandem runs
whose hundreds of rows cross waves and workgroups."""
import functools

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows
from loci_model import loci
from pairs_case import EXACT, K, M, SAME, SETTINGS, SIGMA, WIDE, check
from pairs_model import pair_count, pairs
from test_golden import limit_rows

pytestmark = pytest.mark.gpu

OFF = dict(hits_in=0, kept=0, pairs=0, batches=0, kernel_ms=0.0)


def case():
    return check()  # (cached; asserts the case before any GPU call)


@functools.lru_cache(maxsize=None)
def want(setting):
    return pairs(case()["want"], M, *setting)


_GPU = {}


def gpu_of(device):
    if device not in _GPU:
        _GPU[device] = sa.BiFMIndex.build(case()["recs"], sigma=SIGMA, device=device)
    return _GPU[device]


class pairs_on:
    """set_pairs(min, max) for a block, off again whatever happens in it."""

    def __init__(self, gpu, setting):
        self.gpu, self.setting = gpu, setting

    def __enter__(self):
        self.gpu.set_pairs(*self.setting)
        return self.gpu

    def __exit__(self, *exc):
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


def check_stats(gpu, rows_in, expect, name):
    st = gpu.pairs_stats()
    assert (st["hits_in"], st["kept"], st["pairs"]) == (len(rows_in), len(expect), pair_count(expect)), (name, st)
    assert st["batches"] >= 1 and st["kernel_ms"] > 0, (name, st)


@pytest.mark.parametrize("batch", ["7", "260", None])
@pytest.mark.parametrize("setting", SETTINGS)
def test_every_entry_point_returns_the_paired_hits(gpu_device, monkeypatch, setting, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    with pairs_on(gpu, setting):
        for name, call in entry_points(gpu, c):
            got = hits_as_rows(call())
            assert np.array_equal(got, want(setting)), (name, len(got), len(want(setting)))
            check_stats(gpu, c["want"], want(setting), name)
            assert gpu.stats()["hits"] == len(want(setting)), name
    # the setting is not left behind: the full multiset again, and the stage's figures are zero
    for name, call in entry_points(gpu, c):
        assert np.array_equal(hits_as_rows(call()), c["want"]), name
        assert gpu.pairs_stats() == OFF, name


def test_ramped_batches_with_loci_and_max_hits_around(gpu_device, monkeypatch):
    """The lower bound within the partner query's segment, with loci and
    --max_hits around it; ramps whose entries are no multiples of 4."""
    monkeypatch.setenv("SAHARA_BATCH", "260")
    monkeypatch.setenv("SAHARA_RAMP", "6:9")
    monkeypatch.setenv("SAHARA_RAMP_END", "30:2")
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    with pairs_on(gpu, WIDE):
        assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), want(WIDE))
        assert gpu.stats()["batches"] >= 6
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=3)),
                              limit_rows(want(WIDE), 3))
        gpu.set_loci(2)
        rep = loci(c["want"], 2)
        assert np.array_equal(hits_as_rows(sa.search_packed_compact(gpu, pk, c["scheme"]).to_hits()), pairs(rep, M, *WIDE))
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=1)),
                              limit_rows(pairs(rep, M, *WIDE), 1))


@pytest.mark.parametrize("batch", ["7", "260"])
@pytest.mark.parametrize("W", [0, 2])
def test_with_loci_the_filter_sees_the_representatives(gpu_device, monkeypatch, W, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    rep = loci(c["want"], W)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for setting in SETTINGS:
        expect = pairs(rep, M, *setting)
        assert 0 < len(expect) < len(rep)
        with pairs_on(gpu, setting):
            gpu.set_loci(W)
            for name, call in entry_points(gpu, c):
                assert np.array_equal(hits_as_rows(call()), expect), (name, setting)
                check_stats(gpu, rep, expect, name)
                assert gpu.loci_stats()["loci"] == len(rep), name
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=1)), limit_rows(expect, 1))


@pytest.mark.parametrize("batch", ["7", "260"])
@pytest.mark.parametrize("n", [1, 3])
def test_max_hits_keeps_the_n_best_paired_positions(gpu_device, monkeypatch, n, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for setting in SETTINGS:
        expect = limit_rows(want(setting), n)
        assert len(expect) < len(want(setting))
        with pairs_on(gpu, setting):
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"], max_hits=n)), expect)
            check_stats(gpu, c["want"], want(setting), "search")
            assert gpu.stats()["hits"] == len(expect)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=n)), expect)
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=n)), expect)


@functools.lru_cache(maxsize=None)
def best_case():
    c = case()
    schemes = [sa.search_scheme("h2-k2", j, j, M) for j in range(K + 1)]
    rows = hits_as_rows(O.search_best(c["ref"], c["pats"], schemes, nthreads=8))
    return schemes, rows


HOST_LOOP = "besthits as a host loop"


@pytest.mark.parametrize("batch", ["7", "260"])
def test_besthits_filters_the_stratum_and_refuses_the_host_loop(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    schemes, rows = best_case()
    expect = pairs(rows, M, *WIDE)
    assert 0 < len(expect) < len(rows)
    pk = sa.pack_reads(c["reads"], SIGMA)
    with pairs_on(gpu, WIDE):
        calls = [("search_best", lambda: sa.search_best(gpu, c["pats"], schemes)),
                 ("search_best_reads", lambda: sa.search_best_reads(gpu, c["reads"], schemes)),
                 ("search_best_packed", lambda: sa.search_best_packed(gpu, pk, schemes)),
                 ("search_best_packed_compact", lambda: sa.search_best_packed_compact(gpu, pk, schemes).to_hits())]
        for name, call in calls:
            assert np.array_equal(hits_as_rows(call()), expect), name
            assert gpu.stats()["best_rounds"] == 3, name
            check_stats(gpu, rows, expect, name)
        monkeypatch.setenv("SAHARA_BEST_HOST", "1")
        for name, call in calls[:3]:
            with pytest.raises(sa.SaharaError, match=HOST_LOOP):
                call()
            monkeypatch.delenv("SAHARA_BEST_HOST")
            assert np.array_equal(hits_as_rows(call()), expect), name  # the next call on the same context
            monkeypatch.setenv("SAHARA_BEST_HOST", "1")
    # with pairs off the host loop is what it was
    assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], schemes)), rows)


def test_multi_part_index_filters_per_part_and_refuses_besthits(gpu_device, monkeypatch):
    """The two records in two parts: each part's pass filters its own hits."""
    c = case()
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "30500")
    gpu = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    monkeypatch.setenv("SAHARA_BATCH", "260")
    try:
        assert gpu.info()["n_parts"] == 2
        pk = sa.pack_reads(c["reads"], SIGMA)
        for setting in (WIDE, SAME):
            gpu.set_pairs(*setting)
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"])), want(setting)), setting
            st = gpu.pairs_stats()
            assert st["hits_in"] == len(c["want"]) and st["kept"] == len(want(setting)), st
            assert st["pairs"] >= pair_count(want(setting))  # (a pair with kept hits in both parts counts in each)
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(setting)), setting
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), want(setting)), setting
            got = hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=3))
            assert np.array_equal(got, limit_rows(want(setting), 3)), setting
            gpu.stage(c["pats"], c["scheme"])
            assert gpu.run() == len(want(setting))
            assert np.array_equal(hits_as_rows(gpu.fetch()), want(setting)), setting
        schemes, rows = best_case()
        with pytest.raises(sa.SaharaError, match=HOST_LOOP):
            sa.search_best_reads(gpu, c["reads"], schemes)
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(SAME))
        gpu.set_pairs(None)
        assert np.array_equal(hits_as_rows(sa.search_best_reads(gpu, c["reads"], schemes)), rows)
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), c["want"])
    finally:
        gpu.close()


def test_overflow_rerun_gives_the_same_rows_and_stats(gpu_device, monkeypatch):
    """A hit buffer of 300 entries: the pipelined pass overflows and is redone
    serially; the stage's figures are those of the batches that count."""
    monkeypatch.setenv("SAHARA_BATCH", "260")
    c = case()
    gpu = gpu_of(gpu_device)
    with pairs_on(gpu, WIDE):
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(WIDE))
        plain = gpu.pairs_stats()
    monkeypatch.setenv("SAHARA_HITCAP", "300")
    monkeypatch.setenv("SAHARA_TASKCAP", "200")
    small = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        small.set_pairs(*WIDE)
        assert np.array_equal(hits_as_rows(sa.search_reads(small, c["reads"], c["scheme"])), want(WIDE))
        st = small.pairs_stats()
        assert small.stats()["pipelined"] == 0  # (the re-run is serial: the overflow happened)
        for f in ("hits_in", "kept", "pairs", "batches"):
            assert st[f] == plain[f], (f, st, plain)
        assert st["kernel_ms"] > 0
    finally:
        small.close()


def test_call_time_refusals_leave_the_context_usable(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    odd = sa.pack_reads(c["reads"][:3], SIGMA)

    def works():
        assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), want(WIDE))

    with pairs_on(gpu, WIDE):
        works()
        for call in (lambda: sa.search(gpu, c["pats"][:6], c["scheme"]),
                     lambda: gpu.stage(c["pats"][:6], c["scheme"]),
                     lambda: sa.search_reads(gpu, c["reads"][:3], c["scheme"]),
                     lambda: sa.search_packed(gpu, odd, c["scheme"]),
                     lambda: sa.search_packed_compact(gpu, odd, c["scheme"]),
                     lambda: sa.search_best(gpu, c["pats"][:6], best_case()[0])):
            with pytest.raises(sa.SaharaError, match="no multiple of 4"):
                call()
            works()
        for call in (lambda: sa.search_reads(gpu, c["reads"], c["scheme"], reverse=False),
                     lambda: sa.search_packed(gpu, pk, c["scheme"], reverse=False),
                     lambda: sa.search_packed_compact(gpu, pk, c["scheme"], reverse=False)):
            with pytest.raises(sa.SaharaError, match="reverse"):
                call()
            works()
        for limit in (6, 10, 4 * 7 + 2):  # a cut inside a pair
            with pytest.raises(sa.SaharaError, match="no multiple of 4"):
                sa.search_reads(gpu, c["reads"], c["scheme"], limit=limit)
            with pytest.raises(sa.SaharaError, match="no multiple of 4"):
                sa.search_packed_compact(gpu, pk, c["scheme"], limit=limit)
            works()
        # a cut between pairs is a call on fewer pairs
        got = hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], limit=4 * 50))
        assert np.array_equal(got, want(WIDE)[want(WIDE)[:, 0] < 200])
        gpu.set_pairs(0, M - 1)
        for call in (lambda: sa.search(gpu, c["pats"], c["scheme"]),
                     lambda: sa.search_packed(gpu, pk, c["scheme"]),
                     lambda: gpu.stage(c["pats"], c["scheme"])):
            with pytest.raises(sa.SaharaError, match="below the pattern length"):
                call()
        # staged with pairs off, run with a setting the staged patterns do not fit
        gpu.set_pairs(None)
        gpu.stage(c["pats"], c["scheme"])
        gpu.set_pairs(0, M - 1)
        with pytest.raises(sa.SaharaError, match="below the pattern length"):
            gpu.run()
        gpu.set_pairs(*WIDE)
        works()
        with pytest.raises(sa.SaharaError, match="min_fragment is above max_fragment"):
            gpu.set_pairs(300, 100)
        works()  # (the refused setting changed nothing)


def test_alignment_takes_the_kept_hits_as_any_hits(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    with pairs_on(gpu, EXACT):
        hits = sa.search(gpu, c["pats"], c["scheme"])
    assert np.array_equal(hits_as_rows(hits), want(EXACT))
    got = sa.align(gpu, c["pats"], hits, edit=True, max_err=K)
    assert len(got) == len(hits)
    assert (got["err"].astype(np.int64) <= K).all()  # one record per kept hit, each aligned within the search's bound
