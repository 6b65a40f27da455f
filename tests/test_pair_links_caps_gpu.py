"""The pair stage's link kernels (csrc/pairs.hip kLinkMates, kLinkWrite) on one
batch of more than CAP = 8192 x 256 rows that keeps more than CAP of them:
both launch at most 8192 workgroups of 256 and walk the rest in a grid-stride
loop, so past CAP a wave makes a second trip.

The layout is tests/stage_caps_case.py's LOCI under Hamming k = 1, as in
tests/test_best_pairs_caps_gpu.py. The model runs once per group type and is
tiled: a pair never leaves its group, and a link's mate is an offset, so the
tiles need no shift. Rows, summary and links are compared bit-exact."""
import numpy as np
import pytest

import sahara_amd as sa
import stage_caps_case as S
from best_pairs_model import stats_of
from pair_links_model import PRIMARY, pair_links
from stage_caps_case import CAP, M, SIGMA
from test_stage_caps_gpu import _ham, _same

pytestmark = pytest.mark.gpu
K, FRAG, DELTA = 1, S.WIDE, 0


def expected(layout):
    per = {typ: pair_links(S.group_rows(typ, K), M, *FRAG, DELTA, 1) for typ in set(layout)}
    rows, _ = S._tile(layout, lambda typ: per[typ][0])
    summary = np.concatenate([per[typ][1] for typ in layout])
    links = np.concatenate([per[typ][2] for typ in layout])
    return rows, summary, links, sum(S.rows_of(layout, K)), per


def test_pair_links_past_the_grid_cap(gpu_device, monkeypatch):
    monkeypatch.delenv("SAHARA_BATCH", raising=False)
    layout = list(S.LOCI)
    rows, summary, links, entering, per = expected(layout)
    assert entering > CAP + 64 * 1024 and 0 < len(rows) < entering and len(links) == len(rows)
    big = per[S.TWINS]
    # the big groups: thousands of kept records on one pair, mates tied within a range, a tie of many (MAPQ 0)
    assert len(big[0]) > 4 * 256 and big[3]["tied"].any() and big[3]["n_best"][0] >= 3
    assert len(rows) > CAP  # the kept records themselves reach past the cap: links are written on the second trip
    gpu = sa.BiFMIndex.build(S.text().records, sigma=SIGMA, device=gpu_device)
    try:
        gpu.set_pairs(*FRAG)
        gpu.set_best_pairs(DELTA)
        gpu.set_pair_links(True)
        _same(sa.search(gpu, S.patterns(layout), _ham(K), edit=False), rows, "search")
        assert gpu.stats()["batches"] == 1
        assert np.array_equal(gpu.pair_summary(), summary)
        got = gpu.pair_links()
        differ = np.flatnonzero(got != links)
        assert len(got) == len(links) and len(differ) == 0, (len(got), len(links), differ[:5], got[differ[:5]],
                                                              links[differ[:5]])
        n_kept, n_pairs, _ = stats_of(rows, summary)
        ls = gpu.pair_links_stats()
        assert (ls["links"], ls["primaries"]) == (n_kept, 2 * n_pairs) and ls["kernel_ms"] > 0, ls
        assert int(((got["flags"] & PRIMARY) != 0).sum()) == 2 * n_pairs
    finally:
        gpu.close()
