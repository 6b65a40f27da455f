"""`sahara search --emit-cigar` on the golden fixture ref_a / reads_a: the CIGAR
is the last column of every line and equals the model's, the other columns and
the unflagged output stay what they are, shards align their own hits."""
import os
import subprocess

import numpy as np
import pytest

import align_model as am
from test_cli import SAHARA, run
from test_golden import CASES, GOLD, IDX, SIGMA, expected, patterns, read_fasta
from test_multi_device import _env, run_env

pytestmark = pytest.mark.gpu

Q = os.path.join(GOLD, "reads_a.fa")
I = os.path.join(GOLD, IDX["a"])


def text_a():
    recs = read_fasta(os.path.join(GOLD, "ref_a.fa"), SIGMA["a"])
    T = am.concat_text(recs)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])])
    return T, starts


def search(out, *args, env=None, index=I):
    rc, so, err = run_env(env or {}, "search", "-q", Q, "-i", index, "-o", out, *args)
    assert rc == 0, err
    return so, open(out).read()


def strip_last_column(text):
    return "".join(ln.rsplit(" ", 1)[0] + "\n" for ln in text.splitlines())


def check_cigars(text, pats, k, edit, with_err):
    T, starts = text_a()
    lines = text.splitlines()
    assert lines
    for ln in lines:
        f = ln.split(" ")
        assert len(f) == (5 if with_err else 4), ln
        q, s, p = int(f[0]), int(f[1]), int(f[2])
        res = am.align(pats[q].tolist(), T, int(starts[s]) + p, k, edit)
        assert res is not None, ln
        assert f[-1] == am.cigar(res[2], pats.shape[1]), ln
        if with_err:
            assert res[0] <= int(f[3]) <= k  # the e column stays the hit's own e
    return len(lines)


@pytest.mark.parametrize("name,extra", [("a_lev_k2", []), ("a_lev_k2", ["--emit-errors"]),
                                        ("a_lev_k2", ["--max_hits", "2", "--emit-errors"]),
                                        ("a_best_k2", ["--emit-errors"]), ("a_lev_k2_pigeon_norev", []),
                                        ("a_ham_k2", ["--emit-errors"])])
def test_emit_cigar_appends_the_models_cigar(name, extra, tmp_path, gpu_device):
    c = CASES[name]
    args = ["-e", c["k"], "-g", c["generator"], "-d", c["metric"], "-m", c["mode"], *extra]
    if not c["reverse"]:
        args.append("--no-reverse")
    so0, plain = search(tmp_path / "plain.txt", *args)
    so1, flagged = search(tmp_path / "cigar.txt", *args, "--emit-cigar")
    # without the flag nothing changes: the same bytes as the flagged file less its last column,
    # the golden hits, and no align line in the stats block
    assert strip_last_column(flagged) == plain
    assert "align time:" not in so0 and "  align time:" in so1
    if "--max_hits" not in extra:
        assert len(plain.splitlines()) == c["hits"]
        if "--emit-errors" in extra:
            rows = np.array([ln.split() for ln in plain.splitlines()], np.uint64)
            assert np.array_equal(rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))], expected(name))
    edit = c["metric"] == "lev" or c["mode"] == "besthits"
    n = check_cigars(flagged, patterns("a", c["reverse"]), c["k"], edit, "--emit-errors" in extra)
    assert n == len(plain.splitlines())
    if c["metric"] == "ham" and c["mode"] == "all":
        for ln in flagged.splitlines():
            assert set(ln.rsplit(" ", 1)[1]) <= set("0123456789=X"), ln


def test_unflagged_run_is_reproducible(tmp_path, gpu_device):
    so0, a = search(tmp_path / "a.txt", "-e", 2, "--emit-errors")
    so1, b = search(tmp_path / "b.txt", "-e", 2, "--emit-errors")
    assert a == b and "align time:" not in so0 + so1


@pytest.mark.parametrize("extra", [[], ["--max_hits", "3"]])
def test_emit_cigar_gpus_3_equals_gpus_1(extra, tmp_path, gpu_device):
    args = ["-e", 2, "--emit-errors", "--emit-cigar", *extra]
    _, one = search(tmp_path / "one.txt", *args)
    so, many = search(tmp_path / "many.txt", *args, "--gpus", 3, env=_env(3))
    assert one == many and len(one.splitlines()) > 50
    assert "  align time:" in so and so.count("  device ") == 3


def test_emit_cigar_refuses_more_errors_than_a_record_holds(tmp_path):
    rc, _, err = run("search", "-q", Q, "-i", I, "-o", tmp_path / "x.txt", "-e", 9, "-g", "backtracking", "--emit-cigar")
    assert rc == 1 and "--emit-cigar" in err and not (tmp_path / "x.txt").exists()


def test_emit_cigar_on_a_multi_part_index(tmp_path, gpu_device):
    ref = tmp_path / "ref_a.fa"
    ref.write_bytes(open(os.path.join(GOLD, "ref_a.fa"), "rb").read())
    p = subprocess.run([SAHARA, "index", str(ref)], env=dict(os.environ, SAHARA_PART_SYMBOLS="1000"),
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    raw = (tmp_path / "ref_a.fa.idx").read_bytes()
    assert int.from_bytes(raw[16:24], "little") == 3  # parts
    args = ["-e", 2, "--emit-errors", "--emit-cigar"]
    _, one = search(tmp_path / "one.txt", *args)
    _, parts = search(tmp_path / "parts.txt", *args, index=tmp_path / "ref_a.fa.idx")
    assert one == parts
