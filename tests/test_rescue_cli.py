"""`sahara search --paired --rescue`: the argument errors that end before the
index is asked and the help text (no GPU needed); and, on a GPU, the planted
case of tests/rescue_case.py written as FASTA: the output is the model's rows
line for line, the stats line counts them, two shards write what one writes,
and --loci and --emit-cigar apply around the rescue."""
import os
import re

import numpy as np
import pytest

from loci_model import loci
from pairs_case import K
from rescue_case import MAIN, check, expect, model
from test_align_cli import strip_last_column
from test_cli import run
from test_golden import GOLD, IDX
from test_multi_device import _env, run_env
from test_pairs_cli import rows_of, write_fasta


def test_cli_argument_errors():
    base = ["search", "-i", os.path.join(GOLD, IDX["a"]), "-q", os.path.join(GOLD, "reads_a.fa")]
    rc, _, err = run(*base, "--rescue", 4)
    assert rc == 1 and "--rescue needs --paired" in err
    rc, _, err = run(*base, "--rescue", 4, "--rescue-anchors", 8)
    assert rc == 1 and "--rescue needs --paired" in err
    rc, _, err = run(*base, "--paired", "--rescue-anchors", 8)
    assert rc == 1 and "--rescue-anchors needs --rescue" in err
    for bad in (0, 9):
        rc, _, err = run(*base, "--paired", "--rescue", bad)
        assert rc == 1 and "--rescue takes 1 to 8 errors" in err
    rc, _, err = run(*base, "--paired", "--rescue")
    assert rc == 1 and "--rescue" in err


def test_help_names_the_flags():
    rc, out, err = run("--help")
    text = out + err
    assert "--rescue <n>" in text and "--rescue-anchors <a>" in text


# ---- on a GPU: the planted case of tests/rescue_case.py through the command line

@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    c = check()
    d = tmp_path_factory.mktemp("rescue_cli")
    ref = write_fasta(d / "ref.fa", c["recs"], "rec")
    rc, _, err = run("index", ref)
    assert rc == 0, err
    return dict(index=ref + ".idx", reads=write_fasta(d / "reads.fa", c["reads"], "read"), dir=d)


def search(files, out, *args, env=None):
    out = str(files["dir"] / out)
    rc, so, err = run_env(env or {}, "search", "-q", files["reads"], "-i", files["index"], "-o", out, "-e", K, "--paired",
                          "--min-fragment", MAIN[0], "--max-fragment", MAIN[1], "--emit-errors", *args)
    assert rc == 0, err
    return so, open(out).read()


@pytest.mark.gpu
def test_rescue_writes_the_models_lines_and_the_stats_line(files):
    for Kr in (3, 8):
        want, st = expect(MAIN, Kr), model(MAIN, Kr)[1]
        so, text = search(files, f"k{Kr}.txt", "--rescue", Kr, "--rescue-anchors", 0)
        assert np.array_equal(rows_of(text), want), Kr  # line for line: the file is in canonical order
        m = re.findall(r"^  rescue:\s+(\d+) mates from (\d+) anchors, (\d+) starts, (\d+) reads capped$", so, re.M)
        assert [tuple(map(int, x)) for x in m] == [(st["rescued"], st["anchors"], st["starts"], 0)], so
    # the default cap of 64 leaves the case's queries alone; one of 8 takes the tandem read out
    _, text = search(files, "default.txt", "--rescue", 8)
    assert np.array_equal(rows_of(text), expect(MAIN, 8))
    so, text = search(files, "cap.txt", "--rescue", 8, "--rescue-anchors", 8)
    assert np.array_equal(rows_of(text), expect(MAIN, 8, 8)) and "1 reads capped" in so
    so, text = search(files, "plain.txt")
    assert "rescue:" not in so and len(rows_of(text)) < len(expect(MAIN, 3))


@pytest.mark.gpu
def test_two_shards_loci_and_cigars(files):
    c = check()
    _, one = search(files, "one.txt", "--rescue", 5)
    so2, two = search(files, "two.txt", "--rescue", 5, "--gpus", 2, env=_env(2))
    assert one == two and np.array_equal(rows_of(one), expect(MAIN, 5)) and so2.count("  device ") == 2
    rep = loci(c["want"], K)
    want = expect(MAIN, 8, rows=rep, key="lociK")
    _, text = search(files, "cigar.txt", "--rescue", 8, "--loci", "--emit-cigar")
    assert np.array_equal(rows_of(strip_last_column(text)), want)
    # every line's CIGAR carries its errors (a locus' representative has its position's least), a rescued one's above -e's
    for ln in text.splitlines():
        err, cig = int(ln.split(" ")[3]), ln.rsplit(" ", 1)[1]
        assert re.fullmatch(r"(\d+[=XID])+", cig), ln
        assert sum(int(n) for n, op in re.findall(r"(\d+)([=XID])", cig) if op != "=") == err, ln
    assert any(int(ln.split(" ")[3]) == 8 for ln in text.splitlines())
