"""`sahara search --loci / --loci-window` on the golden fixture ref_a / reads_a:
the output is loci_model.loci of the golden hits line for line, the other
flags apply to the surviving lines, and a run without the flags is what it was."""
import os
import re

import numpy as np
import pytest

from loci_model import loci
from test_align_cli import check_cigars, search, strip_last_column
from test_golden import GOLD, expected, limit_rows, patterns
from test_multi_device import _env

pytestmark = pytest.mark.gpu


def rows_of(text, cols=4):
    return np.array([ln.split(" ") for ln in text.splitlines()], np.uint64).reshape(-1, cols)


def loci_line(so):
    m = re.findall(r"^  loci:\s+(\d+) of (\d+) hits$", so, re.M)
    assert len(m) == 1, so
    return int(m[0][0]), int(m[0][1])


def test_loci_takes_the_error_bound_as_window(tmp_path, gpu_device):
    gold = expected("a_lev_k2")
    want = loci(gold, 2)
    assert 0 < len(want) < len(gold)
    so, text = search(tmp_path / "h.txt", "-e", 2, "--emit-errors", "--loci")
    assert np.array_equal(rows_of(text), want)  # line for line: the file is in canonical order
    assert loci_line(so) == (len(want), len(gold))
    assert f"  number of hits:      {len(want):>10}" in so
    # without --emit-errors: the same lines less the e column
    _, text3 = search(tmp_path / "h3.txt", "-e", 2, "--loci")
    assert np.array_equal(rows_of(text3, 3), want[:, :3])


def test_loci_window_overrides_and_implies(tmp_path, gpu_device):
    gold = expected("a_lev_k2")
    for W in (0, 5):
        so, text = search(tmp_path / f"w{W}.txt", "-e", 2, "--emit-errors", "--loci-window", W)
        assert np.array_equal(rows_of(text), loci(gold, W)), W
        assert loci_line(so) == (len(loci(gold, W)), len(gold))
    _, both = search(tmp_path / "both.txt", "-e", 2, "--emit-errors", "--loci", "--loci-window", 0)
    assert np.array_equal(rows_of(both), loci(gold, 0))
    assert len(loci(gold, 0)) > len(loci(gold, 2)) > len(loci(gold, 5))


def test_max_hits_keeps_the_best_loci(tmp_path, gpu_device):
    want = limit_rows(loci(expected("a_lev_k2"), 2), 2)
    so, text = search(tmp_path / "h.txt", "-e", 2, "--loci", "--max_hits", 2, "--emit-errors")
    assert np.array_equal(rows_of(text), want)
    assert loci_line(so) == (len(loci(expected("a_lev_k2"), 2)), len(expected("a_lev_k2")))


def test_emit_cigar_aligns_the_surviving_lines(tmp_path, gpu_device):
    want = loci(expected("a_lev_k2"), 2)
    _, text = search(tmp_path / "h.txt", "-e", 2, "--loci", "--emit-errors", "--emit-cigar")
    assert np.array_equal(rows_of(strip_last_column(text)), want)
    assert check_cigars(text, patterns("a"), 2, True, True) == len(want)


def test_besthits(tmp_path, gpu_device):
    gold = expected("a_best_k2")
    want = loci(gold, 2)
    so, text = search(tmp_path / "h.txt", "-e", 2, "-m", "besthits", "--loci", "--emit-errors")
    assert np.array_equal(rows_of(text), want)
    assert loci_line(so) == (len(want), len(gold))


def test_two_shards(tmp_path, gpu_device):
    gold = expected("a_lev_k2")
    so, text = search(tmp_path / "h.txt", "-e", 2, "--loci", "--emit-errors", "--gpus", 2, env=_env(2))
    assert np.array_equal(rows_of(text), loci(gold, 2))
    assert loci_line(so) == (len(loci(gold, 2)), len(gold)) and so.count("  device ") == 2


def test_without_the_flags_nothing_changes(tmp_path, gpu_device):
    so, text = search(tmp_path / "h.txt", "-e", 2, "--emit-errors")
    assert text == open(os.path.join(GOLD, "hits_a_lev_k2.txt")).read()
    assert "loci:" not in so
