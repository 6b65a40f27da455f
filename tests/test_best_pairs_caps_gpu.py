"""The pair stage's best mode (csrc/pairs.hip kBestBlocks, kBestScore,
kBestFlags) on one batch of more than CAP = 8192 x 256 rows: each of these
kernels launches at most 8192 workgroups of 256 and walks the rest in a
grid-stride loop, so past CAP a wave makes a second trip.

The layout is tests/stage_caps_case.py's LOCI (598 groups of four queries over
the planted text, 550 of them with 2048 exact copies and 7 copies with one
substitution per mate) under Hamming k = 1, so that scores differ. The model
runs once per group type and is tiled: a pair never leaves its group. Rows,
figures and summary are compared bit-exact. (kBestSummary has no grid cap:
its launch holds one lane per pair of the batch, whatever SAHARA_BATCH is, and
the kernel has no loop.)"""
import numpy as np
import pytest

import sahara_amd as sa
import stage_caps_case as S
from best_pairs_model import best_pairs, stats_of
from pairs_model import pairs
from stage_caps_case import CAP, M, SIGMA
from test_stage_caps_gpu import _ham, _same

pytestmark = pytest.mark.gpu
K, FRAG, DELTA = 1, S.WIDE, 0


def expected(layout):
    per = {typ: best_pairs(S.group_rows(typ, K), M, *FRAG, DELTA, 1) for typ in set(layout)}
    rows, _ = S._tile(layout, lambda typ: per[typ][0])
    summary = np.concatenate([per[typ][1] for typ in layout])
    return rows, summary, sum(S.rows_of(layout, K))


def test_best_pairs_past_the_grid_cap(gpu_device, monkeypatch):
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    layout = list(S.LOCI)
    rows, summary, entering = expected(layout)
    assert entering > CAP + 64 * 1024 and 0 < len(rows) < entering
    big = best_pairs(S.group_rows(S.TWINS, K), M, *FRAG, DELTA, 1)
    paired = pairs(S.group_rows(S.TWINS, K), M, *FRAG)
    assert 0 < len(big[0]) < len(np.unique(paired[:, :3], axis=0))  # the rule drops dearer placements, not only duplicates
    assert big[1]["n_fwd"][0] > 256 and big[1]["next"][0] == 1
    sch = _ham(K)
    pats = S.patterns(layout)
    gpu = sa.BiFMIndex.build(S.text().records, sigma=SIGMA, device=gpu_device)
    try:
        gpu.set_pairs(*FRAG)
        gpu.set_best_pairs(DELTA)
        _same(sa.search(gpu, pats, sch, edit=False), rows, "search")
        assert gpu.stats()["batches"] == 1
        assert np.array_equal(gpu.pair_summary(), summary)
        st = gpu.best_pairs_stats()
        assert (st["hits_in"], st["kept"], st["pairs"], st["unique_pairs"]) == (entering,) + stats_of(rows, summary), st
        ps = gpu.pairs_stats()
        assert (ps["hits_in"], ps["kept"], ps["pairs"]) == (entering, len(rows), st["pairs"]), ps
        pk = sa.pack_reads(S.reads(layout), SIGMA)
        c = sa.search_packed_compact(gpu, pk, sch, edit=False)
        try:
            _same(c.to_hits(), rows, "search_packed_compact")
        finally:
            c.close()
        assert np.array_equal(gpu.pair_summary(), summary)
    finally:
        gpu.close()
