"""`sahara search -m besthits` over the packed besthits calls (2-bit FASTA
ingest, the schemes as rounds on the device): the golden lines, and every
flag that changes the query list against the Python search_best on the same
inputs."""
import os

import numpy as np
import pytest

import sahara_amd as sa
from helpers import hits_as_rows
from test_cli import run
from test_golden import GOLD, IDX, patterns
from test_multi_device import _env, run_env

pytestmark = pytest.mark.gpu

Q = os.path.join(GOLD, "reads_a.fa")
I = os.path.join(GOLD, IDX["a"])
BASE = ["search", "-q", Q, "-i", I, "-e", 2, "-g", "h2-k2", "-m", "besthits", "--emit-errors"]


def _lines(rows):
    return sorted("%d %d %d %d" % (q, s, p, e) for q, s, p, e in np.asarray(rows).tolist())


def test_default_flags_reproduce_the_golden_lines(tmp_path, gpu_device):
    out = tmp_path / "hits.txt"
    rc, so, err = run(*BASE, "-o", out)
    assert rc == 0, err
    want = sorted(open(os.path.join(GOLD, "hits_a_best_k2.txt")).read().splitlines())
    assert sorted(open(out).read().splitlines()) == want
    assert "  search mode:         besthits" in so
    assert sum(line.startswith("node count: ") for line in so.splitlines()) == 3
    # compact records and whole hits give the same file
    full = tmp_path / "full.txt"
    rc, _, err = run_env({"SAHARA_CLI_FULL_HITS": "1"}, *BASE, "-o", full)
    assert rc == 0, err
    assert open(full).read() == open(out).read()


@pytest.mark.parametrize("flags", [["--no-reverse"], ["--limit_queries", 7], ["--max_hits", 2], ["--gpus", 2]],
                         ids=lambda f: str(f[0]).strip("-"))
def test_flags_equal_python_search_best(flags, tmp_path, gpu_device):
    out = tmp_path / "hits.txt"
    rc, _, err = run_env(_env(2) if flags[0] == "--gpus" else {}, *BASE, "-o", out, *flags)
    assert rc == 0, err
    pats = patterns("a", reverse=flags[0] != "--no-reverse")
    if flags[0] == "--limit_queries":
        pats = pats[:7]
    idx = sa.BiFMIndex.load(I, device=gpu_device)
    schemes = [sa.search_scheme("h2-k2", j, j, pats.shape[1]) for j in range(3)]
    want = sa.search_best(idx, pats, schemes, max_hits=2 if flags[0] == "--max_hits" else 0)
    idx.close()
    assert len(want)
    assert sorted(open(out).read().splitlines()) == _lines(hits_as_rows(want))
