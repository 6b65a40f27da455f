"""The paired chain on the device (csrc/pairs.hip, csrc/rescue.hip) at the
grid points of tests/paired_grid_case.py, against the models on the oracle's
rows, bit for bit: pattern lengths of one block, of full blocks and of one
symbol past a block (the rescue's scan reads the block after the partner's
pattern: the next pair's, or with one pair per batch nothing), both
alphabets, K = 1 and 3, the widest window, and some forty records of which
most are shorter than a window, a fragment or the pattern. Every point runs
as one batch and as one pair per batch, through the whole-hit route and the
compact one."""
import numpy as np
import pytest

import sahara_amd as sa
from helpers import hits_as_rows
from paired_grid_case import GRID, WIDEST, check, links, name, rescued, rows_in
from pairs_model import pair_count, pairs
from test_pair_links_gpu import check_call
from test_rescue_gpu import COUNTS

pytestmark = pytest.mark.gpu

BATCHES = ("7", None)  # one pair per batch (the pair stage's granularity is 4: the partner is the batch's last pattern); one batch
every_point = pytest.mark.parametrize("world", GRID, indirect=True, ids=name)


@pytest.fixture(scope="module")
def world(request, gpu_device):
    """(the point, its case, its index on the device): one index at a time, closed when the point's tests are done."""
    point = request.param
    c = check(point)  # (cached; asserts the case before any GPU call)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=point.sigma, device=gpu_device)
    try:
        yield point, c, gpu
    finally:
        gpu.close()


class stages:
    """The chain's stages on for a block, all off again whatever happens in it."""

    def __init__(self, gpu, point, rescue=False, delta=None, loci=None):
        self.gpu, self.point, self.rescue, self.delta, self.loci = gpu, point, rescue, delta, loci

    def __enter__(self):
        self.gpu.set_pairs(*self.point.frag)
        if self.rescue:
            self.gpu.set_rescue(self.point.Kr, 0)
        if self.delta is not None:
            self.gpu.set_best_pairs(self.delta)
            self.gpu.set_pair_links(True)
        if self.loci is not None:
            self.gpu.set_loci(self.loci)
        return self.gpu

    def __exit__(self, *exc):
        self.gpu.set_pair_links(False)
        self.gpu.set_best_pairs(None)
        self.gpu.set_rescue(None)
        self.gpu.set_pairs(None)
        self.gpu.set_loci(None)


def entry_points(gpu, c):
    point = c["point"]
    pk = sa.pack_reads(c["reads"], point.sigma)
    yield "search", lambda: sa.search(gpu, c["pats"], c["scheme"], edit=point.edit)
    yield "search_packed_compact", lambda: sa.search_packed_compact(gpu, pk, c["scheme"], edit=point.edit).to_hits()


def set_batch(monkeypatch, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    else:
        monkeypatch.delenv("SAHARA_BATCH", raising=False)


@every_point
@pytest.mark.parametrize("batch", BATCHES)
def test_pairs_alone(world, monkeypatch, batch):
    set_batch(monkeypatch, batch)
    point, c, gpu = world
    want = pairs(c["want"], point.M, *point.frag)
    with stages(gpu, point):
        for name_, call in entry_points(gpu, c):
            got = hits_as_rows(call())
            assert np.array_equal(got, want), (name_, len(got), len(want))
            ps = gpu.pairs_stats()
            assert (ps["hits_in"], ps["kept"], ps["pairs"]) == (len(c["want"]), len(want), pair_count(want)), (name_, ps)
    # all off again: the call is what it was
    assert np.array_equal(hits_as_rows(sa.search(gpu, c["pats"], c["scheme"], edit=point.edit)), c["want"])


@every_point
@pytest.mark.parametrize("batch", BATCHES)
def test_pairs_and_rescue(world, monkeypatch, batch):
    set_batch(monkeypatch, batch)
    point, c, gpu = world
    rows, counts = rescued(point)
    want = pairs(rows, point.M, *point.frag)
    with stages(gpu, point, rescue=True):
        for name_, call in entry_points(gpu, c):
            got = hits_as_rows(call())
            assert np.array_equal(got, want), (name_, len(got), len(want))
            st = gpu.rescue_stats()
            assert {f: st[f] for f in COUNTS} == {f: counts[f] for f in COUNTS}, (name_, st, counts)
            ps = gpu.pairs_stats()
            assert (ps["hits_in"], ps["kept"], ps["pairs"]) == (len(rows), len(want), pair_count(want)), (name_, ps)
            # what the batch setting is here for: every pair is a batch of its own, so the partner of read A's
            # forward anchor (qid 4P + 3) is its batch's last pattern: the block after it lies past the descriptor
            assert gpu.stats()["batches"] == (c["n_pairs"] if batch else 1), (name_, gpu.stats()["batches"])


@every_point
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("delta", [0, 1])
def test_rescue_best_pairs_and_links(world, monkeypatch, delta, batch):
    set_batch(monkeypatch, batch)
    point, c, gpu = world
    rows, counts = rescued(point)
    with stages(gpu, point, rescue=True, delta=delta):
        for name_, call in entry_points(gpu, c):
            check_call(gpu, call(), rows, links(point, delta), (name_, delta))
            st = gpu.rescue_stats()
            assert {f: st[f] for f in COUNTS} == {f: counts[f] for f in COUNTS}, (name_, st, counts)


@pytest.mark.parametrize("world", [WIDEST], indirect=True, ids=name)
@pytest.mark.parametrize("batch", BATCHES)
def test_with_loci_the_chain_runs_over_the_representatives(world, monkeypatch, batch):
    set_batch(monkeypatch, batch)
    point, c, gpu = world
    rep = rows_in(point, 2)
    rows, counts = rescued(point, 2)
    assert len(rep) < len(c["want"]) and counts["rescued"] > 0
    for delta in (0, 1):
        model = links(point, delta, 2)
        assert len(model[0])
        with stages(gpu, point, rescue=True, delta=delta, loci=2):
            for name_, call in entry_points(gpu, c):
                check_call(gpu, call(), rows, model, (name_, delta))
                st = gpu.rescue_stats()
                assert {f: st[f] for f in COUNTS} == {f: counts[f] for f in COUNTS}, (name_, st, counts)
                assert gpu.loci_stats()["loci"] == len(rep), name_
