"""`sahara search --paired` on the planted case of tests/pairs_case.py, its
records and reads written as FASTA: the output is pairs_model.pairs of the
oracle's rows line for line, the stats line counts them, shards hold whole
pairs, and the other flags apply to the kept lines."""
import functools
import os
import re

import numpy as np
import pytest

from loci_model import loci
from pairs_case import K, M, SIGMA, WIDE, check
from pairs_model import pair_count, pairs
from test_align_cli import strip_last_column
from test_cli import run
from test_golden import CHARS
from test_multi_device import _env, run_env

pytestmark = pytest.mark.gpu


def write_fasta(path, rows, name):
    letters = np.frombuffer(CHARS[SIGMA].encode(), np.uint8)
    with open(path, "w") as f:
        for i, r in enumerate(rows):
            f.write(f">{name}{i}\n{letters[np.asarray(r)].tobytes().decode()}\n")
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    c = check()
    d = tmp_path_factory.mktemp("pairs_cli")
    ref = write_fasta(d / "ref.fa", c["recs"], "rec")
    rc, _, err = run("index", ref)
    assert rc == 0, err
    return dict(index=ref + ".idx", reads=write_fasta(d / "reads.fa", c["reads"], "read"),
                fewer=write_fasta(d / "fewer.fa", c["reads"][:2 * 237], "read"), dir=d)


def search(files, out, *args, reads="reads", env=None):
    out = str(files["dir"] / out)
    rc, so, err = run_env(env or {}, "search", "-q", files[reads], "-i", files["index"], "-o", out, "-e", K, *args)
    assert rc == 0, err
    return so, open(out).read()


def rows_of(text, cols=4):
    return np.array([ln.split(" ") for ln in text.splitlines()], np.uint64).reshape(-1, cols)


def pairs_line(so):
    m = re.findall(r"^  pairs:\s+(\d+) of (\d+) hits, (\d+) pairs$", so, re.M)
    assert len(m) == 1, so
    return tuple(int(x) for x in m[0])


def test_paired_writes_the_models_lines_and_the_stats_line(files):
    w = check()["want"]
    want = pairs(w, M, *WIDE)
    so, text = search(files, "wide.txt", "--emit-errors", "--paired", "--min-fragment", WIDE[0], "--max-fragment", WIDE[1])
    assert np.array_equal(rows_of(text), want)  # line for line: the file is in canonical order
    assert pairs_line(so) == (len(want), len(w), pair_count(want))
    assert f"  number of hits:      {len(want):>10}" in so
    # the defaults: fragments 0 .. 500
    so, text = search(files, "default.txt", "--emit-errors", "--paired")
    assert np.array_equal(rows_of(text), pairs(w, M, 0, 500))
    assert pairs_line(so)[0] == len(pairs(w, M, 0, 500)) > len(want)
    # without the flag the run is what it was
    so, text = search(files, "plain.txt", "--emit-errors")
    assert np.array_equal(rows_of(text), w) and "pairs:" not in so


def test_two_shards_of_an_odd_number_of_pairs_write_what_one_writes(files):
    w = check()["want"]
    want = pairs(w[w[:, 0] < 4 * 237], M, *WIDE)
    frag = ("--paired", "--min-fragment", WIDE[0], "--max-fragment", WIDE[1], "--emit-errors")
    so1, one = search(files, "one.txt", *frag, reads="fewer")
    so2, two = search(files, "two.txt", *frag, "--gpus", 2, reads="fewer", env=_env(2))
    assert one == two and np.array_equal(rows_of(one), want)
    assert pairs_line(so1) == pairs_line(so2) and so2.count("  device ") == 2


def test_loci_and_cigars_on_the_kept_lines(files):
    want = pairs(loci(check()["want"], K), M, *WIDE)
    _, text = search(files, "cigar.txt", "--paired", "--min-fragment", WIDE[0], "--max-fragment", WIDE[1], "--loci",
                     "--emit-errors", "--emit-cigar")
    assert np.array_equal(rows_of(strip_last_column(text)), want)
    cigars = [ln.rsplit(" ", 1)[1] for ln in text.splitlines()]
    assert len(cigars) == len(want) and all(re.fullmatch(r"(\d+[=XID])+", x) for x in cigars)
