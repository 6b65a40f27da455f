"""The loci stage on the device (csrc/loci.hip; docs/semantics.md "Loci")
against tests/loci_model.py: every call equals loci(oracle rows, W), compared
bit-exact as sorted rows, on the planted case of tests/loci_case.py: copies of
a segment (two of them 157 apart, two in the other record), tandem runs and a
homopolymer, so that queries have several loci, loci hold thousands of records
across waves and workgroups, and the least e of a locus sits at several
positions."""
import functools

import numpy as np
import pytest

import align_model as am
import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows
from loci_case import K, M, SIGMA, planted
from loci_model import loci, locus_ids
from test_golden import limit_rows

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case():
    """The planted case, with what the tests below rely on asserted on the
    oracle's rows before any GPU call."""
    c = planted()
    w = c["want"]
    counts = [len(want(W)) for W in range(7)]
    assert len(set(counts)) == 7, counts
    ids = locus_ids(w, 2)
    first = np.flatnonzero(np.diff(ids, prepend=-1))
    last = np.append(first[1:], len(w))
    tied = big = 0
    for a, b in zip(first.tolist(), last.tolist()):
        r = w[a:b]
        big += b - a >= 256
        tied += len(np.unique(r[r[:, 3] == r[:, 3].min(), 2])) >= 2
    assert tied >= 20, tied
    assert big >= 5, big
    assert (np.unique(want(2)[:, 0], return_counts=True)[1] > 1).sum() >= 50
    both = sum(len(np.unique(w[w[:, 0] == q, 1])) > 1 for q in np.unique(w[:, 0]))
    assert both >= 10, both
    assert len(w) <= 2_000_000
    return c


@functools.lru_cache(maxsize=None)
def want(W):
    return loci(planted()["want"], W)


_GPU = {}


def gpu_of(device):
    if device not in _GPU:
        _GPU[device] = sa.BiFMIndex.build(case()["recs"], sigma=SIGMA, device=device)
    return _GPU[device]


class loci_on:
    """set_loci(W) for a block, off again whatever happens in it."""

    def __init__(self, gpu, W):
        self.gpu, self.W = gpu, W

    def __enter__(self):
        self.gpu.set_loci(self.W)
        return self.gpu

    def __exit__(self, *exc):
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


@pytest.mark.parametrize("batch", ["7", "257", None])
@pytest.mark.parametrize("W", [0, 2, 5])
def test_every_entry_point_returns_the_loci(gpu_device, monkeypatch, W, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    with loci_on(gpu, W):
        for name, call in entry_points(gpu, c):
            got = hits_as_rows(call())
            assert np.array_equal(got, want(W)), (name, len(got), len(want(W)))
            st = gpu.loci_stats()
            assert st["hits_in"] == len(c["want"]) and st["loci"] == len(want(W)), (name, st)
            assert st["batches"] >= 1 and st["kernel_ms"] > 0, (name, st)
            assert gpu.stats()["hits"] == len(want(W)), name
    # the setting is not left behind: the full multiset again, and the stage's figures are zero
    for name, call in entry_points(gpu, c):
        assert np.array_equal(hits_as_rows(call()), c["want"]), name
        assert gpu.loci_stats() == dict(hits_in=0, loci=0, batches=0, kernel_ms=0.0), name


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W", [0, 2])
def test_max_hits_keeps_the_n_best_loci(gpu_device, monkeypatch, W, n):
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = case()
    gpu = gpu_of(gpu_device)
    expect = limit_rows(want(W), n)
    assert len(expect) < len(want(W))
    pk = sa.pack_reads(c["reads"], SIGMA)
    with loci_on(gpu, W):
        assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"], max_hits=n)), expect)
        assert gpu.loci_stats()["loci"] == len(want(W)) and gpu.stats()["hits"] == len(expect)
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=n)), expect)
        assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=n)), expect)


@functools.lru_cache(maxsize=None)
def best_case():
    c = case()
    schemes = [sa.search_scheme("h2-k2", j, j, M) for j in range(K + 1)]
    rows = hits_as_rows(O.search_best(c["ref"], c["pats"], schemes, nthreads=8))
    return schemes, rows


@pytest.mark.parametrize("batch", ["7", "257"])
def test_besthits_filters_the_stratum(gpu_device, monkeypatch, batch):
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = case()
    gpu = gpu_of(gpu_device)
    schemes, rows = best_case()
    W = 2
    expect = loci(rows, W)
    assert len(expect) < len(rows) and set(expect[:, 0].tolist()) == set(rows[:, 0].tolist())
    pk = sa.pack_reads(c["reads"], SIGMA)
    with loci_on(gpu, W):
        calls = [("search_best", lambda: sa.search_best(gpu, c["pats"], schemes)),
                 ("search_best_reads", lambda: sa.search_best_reads(gpu, c["reads"], schemes)),
                 ("search_best_packed", lambda: sa.search_best_packed(gpu, pk, schemes)),
                 ("search_best_packed_compact", lambda: sa.search_best_packed_compact(gpu, pk, schemes).to_hits())]
        for name, call in calls:
            assert np.array_equal(hits_as_rows(call()), expect), name
            assert gpu.stats()["best_rounds"] == 3, name
            st = gpu.loci_stats()
            assert st["hits_in"] == len(rows) and st["loci"] == len(expect), (name, st)
        assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], schemes, max_hits=1)), limit_rows(expect, 1))
        monkeypatch.setenv("SAHARA_BEST_HOST", "1")
        for name, call in calls[:3]:
            assert np.array_equal(hits_as_rows(call()), expect), name
            assert gpu.stats()["best_rounds"] == 0, name
            st = gpu.loci_stats()
            assert st["hits_in"] == len(rows) and st["loci"] == len(expect), (name, st)
        assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], schemes, max_hits=3)), limit_rows(expect, 3))


def test_multi_part_index_filters_per_part(gpu_device, monkeypatch):
    """The two records in two parts: each part's pass filters its own hits,
    --max_hits then runs on the host over the merged representatives."""
    c = case()
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "6500")
    gpu = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    monkeypatch.setenv("SAHARA_BATCH", "257")
    try:
        assert gpu.info()["n_parts"] == 2
        pk = sa.pack_reads(c["reads"], SIGMA)
        for W in (0, 2):
            gpu.set_loci(W)
            assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"])), want(W)), W
            st = gpu.loci_stats()
            assert st["hits_in"] == len(c["want"]) and st["loci"] == len(want(W)), st
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(W)), W
            assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"])), want(W)), W
            for n in (1, 3):
                got = hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"], max_hits=n))
                assert np.array_equal(got, limit_rows(want(W), n)), (W, n)
            gpu.stage(c["pats"], c["scheme"])
            assert gpu.run() == len(want(W))
            assert np.array_equal(hits_as_rows(gpu.fetch()), want(W)), W
        schemes, rows = best_case()
        assert np.array_equal(hits_as_rows(sa.search_best_reads(gpu, c["reads"], schemes)), loci(rows, 2))
        gpu.set_loci(None)
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), c["want"])
    finally:
        gpu.close()


@pytest.mark.parametrize("route", ["SAHARA_FULL_DOWNLOAD", "SAHARA_COMPACT_DOWNLOAD"])
def test_forced_routes(gpu_device, monkeypatch, route):
    """Whole hits by DMA into a pinned sink, and 8-B records through the
    download ring with the whole-hit fallback: the sink is pinned from the
    second call of a size on."""
    monkeypatch.setenv("SAHARA_BATCH", "257")
    monkeypatch.setenv("SAHARA_PIN_MIN", "0")
    monkeypatch.setenv(route, "1")
    c = case()
    gpu = gpu_of(gpu_device)
    pk = sa.pack_reads(c["reads"], SIGMA)
    for W in (0, 2):
        with loci_on(gpu, W):
            for _ in range(2):
                assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(W)), W
                assert np.array_equal(hits_as_rows(sa.search_packed(gpu, pk, c["scheme"], max_hits=3)),
                                      limit_rows(want(W), 3)), W
    assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), c["want"])


def test_compact_call_whose_sink_is_too_small(gpu_device, monkeypatch):
    """A first compact call on a fresh context with a sink of 300 records
    (SAHARA_SINK_RECORDS, a test hook): the sink falls out of step, and the
    records of every batch are made again after the pass from the whole hits
    the device kept, which are the filtered ones."""
    monkeypatch.setenv("SAHARA_BATCH", "57")
    monkeypatch.setenv("SAHARA_SINK_RECORDS", "300")
    c = case()
    gpu = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        pk = sa.pack_reads(c["reads"], SIGMA)
        for W in (0, 2):
            assert len(want(W)) > 300
            gpu.set_loci(W)
            h = sa.search_packed_compact(gpu, pk, c["scheme"])
            assert np.array_equal(hits_as_rows(h.to_hits()), want(W)), W
            h.close()
        gpu.set_loci(None)
        h = sa.search_packed_compact(gpu, pk, c["scheme"])
        assert np.array_equal(hits_as_rows(h.to_hits()), c["want"])
        h.close()
    finally:
        gpu.close()


def test_overflow_rerun_gives_the_same_rows_and_stats(gpu_device, monkeypatch):
    """A hit buffer of 300 entries: the pipelined pass overflows and is redone
    serially; the stage's figures are those of the batches that count."""
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = case()
    gpu = gpu_of(gpu_device)
    with loci_on(gpu, 2):
        assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(2))
        plain = gpu.loci_stats()
    monkeypatch.setenv("SAHARA_HITCAP", "300")
    monkeypatch.setenv("SAHARA_TASKCAP", "200")
    small = sa.BiFMIndex.build(c["recs"], sigma=SIGMA, device=gpu_device)
    try:
        small.set_loci(2)
        assert np.array_equal(hits_as_rows(sa.search_reads(small, c["reads"], c["scheme"])), want(2))
        st = small.loci_stats()
        assert small.stats()["pipelined"] == 0  # (the re-run is serial: the overflow happened)
        for f in ("hits_in", "loci", "batches"):
            assert st[f] == plain[f], (f, st, plain)
        assert st["kernel_ms"] > 0
    finally:
        small.close()


def test_fm_only_chain(gpu_device, monkeypatch):
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = case()
    gpu = gpu_of(gpu_device)
    try:
        gpu.set_mode(verify=False, locate_sa=False)
        with loci_on(gpu, 2):
            assert np.array_equal(hits_as_rows(sa.search_reads(gpu, c["reads"], c["scheme"])), want(2))
            assert gpu.loci_stats()["hits_in"] == len(c["want"])
    finally:
        gpu.set_mode(verify=True, locate_sa=True)


def test_alignment_takes_the_loci_as_any_hits(gpu_device):
    c = case()
    gpu = gpu_of(gpu_device)
    with loci_on(gpu, 2):
        hits = sa.search(gpu, c["pats"], c["scheme"])
    assert np.array_equal(hits_as_rows(hits), want(2))
    got = sa.align(gpu, c["pats"], hits, edit=True, max_err=K)
    T = am.concat_text(c["recs"])
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in c["recs"]])]).astype(np.int64)
    assert len(got) == len(hits)
    for r, h in zip(got, hits):
        res = am.align(c["pats"][int(h["qid"])].tolist(), T, int(starts[int(h["seq_id"])]) + int(h["pos"]), K, True)
        assert (int(r["err"]), int(r["ref_len"]), r["edit"].tolist()) == am.record_of(res), (h, r)
        assert int(r["err"]) == int(h["err"])  # the representative's err is its position's least e
