"""`sahara search --paired --best-pairs` on the planted case of
tests/best_pairs_case.py, its records and reads written as FASTA: the output
is best_pairs_model.best_pairs of the oracle's rows line for line, the stats
line counts them, the summary file holds the model's summary, and two shards
write what one writes."""
import re

import numpy as np
import pytest

from best_pairs_case import K, WIDE, check, expected
from best_pairs_model import NONE, stats_of
from test_cli import run
from test_multi_device import _env, run_env
from test_pairs_cli import rows_of, write_fasta

pytestmark = pytest.mark.gpu
FRAG = ("--paired", "--min-fragment", WIDE[0], "--max-fragment", WIDE[1], "--emit-errors")


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    c = check()
    d = tmp_path_factory.mktemp("best_pairs_cli")
    ref = write_fasta(d / "ref.fa", c["recs"], "rec")
    rc, _, err = run("index", ref)
    assert rc == 0, err
    return dict(index=ref + ".idx", reads=write_fasta(d / "reads.fa", c["reads"], "read"), dir=d)


def search(files, out, *args, env=None):
    out = str(files["dir"] / out)
    rc, so, err = run_env(env or {}, "search", "-q", files["reads"], "-i", files["index"], "-o", out, "-e", K, *args)
    assert rc == 0, err
    return so, open(out).read()


def best_line(so):
    m = re.findall(r"^  best pairs:\s+(\d+) of (\d+) hits, (\d+) pairs, (\d+) unique \(delta (\d+)\)$", so, re.M)
    assert len(m) == 1, so
    return tuple(int(x) for x in m[0])


def summary_lines(summary):
    return "".join(f"{p}\t{x['best']}\t{x['next']}\t{x['n_fwd']}\t{x['n_rev']}\n"
                   for p, x in enumerate(summary) if x["best"] != NONE)


@pytest.mark.parametrize("delta", [0, 1])
def test_best_pairs_writes_the_models_lines_the_stats_line_and_the_summary(files, delta):
    w = check()["want"]
    kept, summary = expected(WIDE, delta)
    tsv = str(files["dir"] / f"summary{delta}.tsv")
    flags = ("--best-pairs", "--pair-summary", tsv) + (("--pair-delta", delta) if delta else ())
    so, text = search(files, f"best{delta}.txt", *FRAG, *flags)
    assert np.array_equal(rows_of(text), kept)  # line for line: the file is in canonical order
    assert best_line(so) == (len(kept), len(w)) + stats_of(kept, summary)[1:] + (delta,)
    assert f"  number of hits:      {len(kept):>10}" in so
    assert open(tsv).read() == summary_lines(summary) != ""
    # without the flag the run is what it was
    so, _ = search(files, "plain.txt", *FRAG)
    assert "best pairs:" not in so


def test_two_shards_write_what_one_writes(files):
    kept, summary = expected(WIDE, 0)
    one, two = str(files["dir"] / "one.tsv"), str(files["dir"] / "two.tsv")
    so1, text1 = search(files, "one.txt", *FRAG, "--best-pairs", "--pair-summary", one)
    so2, text2 = search(files, "two.txt", *FRAG, "--best-pairs", "--pair-summary", two, "--gpus", 2, env=_env(2))
    assert text1 == text2 and np.array_equal(rows_of(text1), kept)
    assert best_line(so1) == best_line(so2) and so2.count("  device ") == 2
    assert open(one).read() == open(two).read() == summary_lines(summary)
