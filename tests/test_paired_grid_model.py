"""tests/paired_grid_case.py on the CPU: every grid point's case still covers
the edge it is in the grid for (check()), and the models of the chain take
the records that no test had before: shorter than the pattern, too short for
a fragment, of one symbol. No GPU: tests/test_paired_grid_gpu.py runs the
points on one."""
import numpy as np
import pytest

from paired_grid_case import GRID, check, dists, links, name, rescued
from pairs_model import pairs
from rescue_model import window


@pytest.mark.parametrize("point", GRID, ids=name)
def test_the_point_covers_its_edge(point):
    check(point)


@pytest.mark.parametrize("point", GRID, ids=name)
def test_the_models_take_records_shorter_than_the_pattern_and_the_fragment(point):
    c = check(point)
    M = point.M
    dmin, dmax = dists(point)
    lens = np.array([len(r) for r in c["recs"]])
    w = c["want"]
    below = lens[w[:, 1].astype(np.int64)] < dmin + M  # rows on records that no fragment fits on
    assert below.any() and (lens < M).any() and (lens == 1).any()
    if point.edit:  # (a pattern of M symbols lies on M - 1 with one of them put in)
        assert (lens[w[:, 1].astype(np.int64)] < M).any()
    # a window on such a record stays on it, or is none
    for q, s, p, _ in w[below].tolist():
        got = window(q, p, dmin, dmax, int(lens[s]))
        assert got is None or 0 <= got[0] <= got[1] <= lens[s] - 1, (q, s, p, got)
    # no stage keeps or adds a row there
    have = set(map(tuple, w.tolist()))
    stages = (pairs(w, M, *point.frag), np.array([r for r in rescued(point)[0].tolist() if tuple(r) not in have]),
              links(point, 0)[0], links(point, 1)[0])
    for rows in stages:
        assert len(rows) and (lens[rows[:, 1].astype(np.int64)] >= dmin + M).all()
