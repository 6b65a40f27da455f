"""`sahara search --paired --best-pairs --sam` on the planted case of
tests/best_pairs_case.py, its records and reads written as FASTA: the file is
tests/sam_model.py's text byte for byte (the model's rows, links and
alignments), two shards write the same bytes, the lines hold together as SAM
whatever the model says, and the flag's refusals; and with --rescue on the
widest-window point of tests/paired_grid_case.py (dna4, patterns of 33
symbols): the alignment bound is max(-e, --rescue)."""
import functools
import re

import numpy as np
import pytest

import paired_grid_case as grid
from best_pairs_case import K, M, SIGMA, WIDE, planted
from loci_model import loci
from pair_links_case import check, expected_links
from pair_links_model import pair_links
from sam_model import sam_text
from test_cli import run
from test_golden import CHARS
from test_multi_device import _env, run_env
from test_pairs_cli import write_fasta

pytestmark = pytest.mark.gpu
FRAG = ("--paired", "--min-fragment", WIDE[0], "--max-fragment", WIDE[1])


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    c = check()
    d = tmp_path_factory.mktemp("sam_cli")
    ref = write_fasta(d / "ref.fa", c["recs"], "rec")
    rc, _, err = run("index", ref)
    assert rc == 0, err
    return dict(index=ref + ".idx", reads=write_fasta(d / "reads.fa", c["reads"], "read"), dir=d)


def search(files, out, *args, env=None):
    out = str(files["dir"] / out)
    rc, so, err = run_env(env or {}, "search", "-q", files["reads"], "-i", files["index"], "-o", out, "-e", K, *args)
    assert rc == 0, err
    return so, open(out).read()


@functools.lru_cache(maxsize=None)
def model_text(delta, W=None):
    c = planted()
    if W is None:
        kept, summary, links, info = expected_links(WIDE, delta)
    else:
        kept, summary, links, info = pair_links(loci(c["want"], W), M, *WIDE, delta, c["n_pairs"])
    return sam_text(c["recs"], c["pats"], SIGMA, kept, links, c["n_pairs"], K), links


def links_line(so):
    m = re.findall(r"^  pair links:\s+(\d+) links, (\d+) primary, (\d+) pairs with MAPQ >= 30$", so, re.M)
    assert len(m) == 1, so
    return tuple(int(x) for x in m[0])


def cigar_lengths(cigar):
    ops = re.findall(r"(\d+)([=XID])", cigar)
    assert "".join(n + o for n, o in ops) == cigar, cigar
    return (sum(int(n) for n, o in ops if o in "=XI"), sum(int(n) for n, o in ops if o in "=XD"))


def check_structure(text, n_pairs, n_records, length):
    """What holds of the file as SAM, whatever the model says; length: the reads'."""
    lines = text.splitlines()
    head = [ln for ln in lines if ln.startswith("@")]
    body = lines[len(head):]
    assert head[0] == "@HD\tVN:1.6\tSO:unsorted\tGO:query" and head[-1] == "@PG\tID:sahara\tPN:sahara"
    assert len(head) == n_records + 2 and all(ln.startswith("@SQ\tSN:") for ln in head[1:-1])
    assert not any(ln.startswith("@") for ln in body)
    by_pair = {}
    for ln in body:
        f = ln.split("\t")
        assert len(f) in (11, 13), ln  # 11 fields, and the two tags of a mapped record
        by_pair.setdefault(int(f[0]), []).append(f)
    assert list(by_pair) == list(range(n_pairs))  # pairs in query order, none missing
    mapped = 0
    for P, fs in by_pair.items():
        if fs[0][2] == "*":  # unmapped: the two reads, flags 77 and 141
            assert [f[1] for f in fs] == ["77", "141"], P
            for f in fs:
                assert f[2:9] == ["*", "0", "0", "*", "*", "0", "0"] and len(f[9]) == length and f[10] == "*" and len(f) == 11
            continue
        mapped += 1
        prim = {0x40: [], 0x80: []}
        for f in fs:
            flag = int(f[1])
            assert len(f) == 13 and flag & 0x3 == 0x3 and bool(flag & 0x10) != bool(flag & 0x20), f
            assert bool(flag & 0x40) != bool(flag & 0x80) and flag & ~0x1F3 == 0, f
            qlen, rlen = cigar_lengths(f[5])
            assert qlen == len(f[9]) == length and set(f[9]) <= set("ACGTN"), f
            assert f[6] == "=" and f[10] == "*" and re.fullmatch(r"NM:i:\d+", f[11]) and re.fullmatch(r"ZP:i:\d+", f[12])
            assert 0 <= int(f[4]) <= 60 and (int(f[4]) == 0 or not flag & 0x100), f
            assert abs(int(f[8])) >= rlen, f
            if not flag & 0x100:
                prim[flag & 0xC0].append(f)
        # exactly one primary line per read; they name each other, and their lengths sum to 0
        assert len(prim[0x40]) == 1 and len(prim[0x80]) == 1, P
        a, b = prim[0x40][0], prim[0x80][0]
        assert a[2] == b[2] and a[7] == b[3] and b[7] == a[3] and int(a[8]) + int(b[8]) == 0 and a[4] == b[4], P
        assert bool(int(a[1]) & 0x10) != bool(int(b[1]) & 0x10), P
    return mapped


@pytest.mark.parametrize("delta", [0, 1])
def test_sam_is_the_models_text(files, delta):
    c = check()
    want, links = model_text(delta)
    flags = ("--best-pairs", "--sam") + (("--pair-delta", delta) if delta else ())
    so, text = search(files, f"out{delta}.sam", *FRAG, *flags)
    assert text == want
    n_prim = int((links["flags"] & 1).sum())
    mapq30 = int(((links["flags"] & 1 != 0) & (links["mapq"] >= 30)).sum()) // 2
    assert links_line(so) == (len(links), n_prim, mapq30)
    assert "  align time:" in so and f"  number of hits:      {len(links):>10}" in so
    assert check_structure(text, c["n_pairs"], len(c["recs"]), M) == n_prim // 2
    assert 0 < n_prim // 2 < c["n_pairs"]  # (the case has pairs that keep nothing)
    # without the flag the run is what it was: the hit lines, no links line
    so, plain = search(files, "plain.txt", *FRAG, *(f for f in flags if f != "--sam"), "--emit-errors")
    assert "pair links:" not in so and not plain.startswith("@") and len(plain.splitlines()) == len(links)


def test_sam_with_loci(files):
    c = check()
    want, links = model_text(0, 2)
    so, text = search(files, "loci.sam", *FRAG, "--best-pairs", "--sam", "--loci-window", 2)
    assert text == want != model_text(0)[0]
    check_structure(text, c["n_pairs"], len(c["recs"]), M)


def test_two_shards_write_the_same_bytes(files):
    c = check()
    so1, one = search(files, "one.sam", *FRAG, "--best-pairs", "--sam")
    so2, two = search(files, "two.sam", *FRAG, "--best-pairs", "--sam", "--gpus", 2, env=_env(2))
    assert one == two == model_text(0)[0]
    assert links_line(so1) == links_line(so2) and so2.count("  device ") == 2


def write_fasta_of(path, rows, name, sigma):
    letters = np.frombuffer(CHARS[sigma].encode(), np.uint8)
    with open(path, "w") as f:
        for i, r in enumerate(rows):
            f.write(f">{name}{i}\n{letters[np.asarray(r)].tobytes().decode()}\n")
    return str(path)


def test_sam_with_rescue(tmp_path, gpu_device):
    """--rescue with --sam on a dna4 index: rescued records carry up to --rescue
    errors, above -e's, and are aligned with the larger bound; records of one
    symbol and the widest fragment window come through the command line."""
    point = grid.WIDEST
    c = grid.check(point)
    kept, summary, links, info = grid.links(point, 0)
    want = sam_text(c["recs"], c["pats"], point.sigma, kept, links, c["n_pairs"], max(point.K, point.Kr))
    ref = write_fasta_of(tmp_path / "ref.fa", c["recs"], "rec", point.sigma)
    rc, _, err = run("index", ref, "--dna4")
    assert rc == 0, err
    out = tmp_path / "rescue.sam"
    rc, so, err = run("search", "-q", write_fasta_of(tmp_path / "reads.fa", c["reads"], "read", point.sigma), "-i",
                      ref + ".dna4.idx", "-o", out, "-e", point.K, "-g", point.generator, "--paired", "--min-fragment",
                      point.frag[0], "--max-fragment", point.frag[1], "--rescue", point.Kr, "--rescue-anchors", 0,
                      "--best-pairs", "--sam")
    assert rc == 0, err
    text = out.read_text()
    assert text == want
    n_prim = int((links["flags"] & 1).sum())
    mapq30 = int(((links["flags"] & 1 != 0) & (links["mapq"] >= 30)).sum()) // 2
    assert links_line(so) == (len(links), n_prim, mapq30)
    assert check_structure(text, c["n_pairs"], len(c["recs"]), point.M) == n_prim // 2
    # rescued records are in the file: lines with more errors than -e allows, up to --rescue's
    nm = [int(x) for x in re.findall(r"\tNM:i:(\d+)\t", text)]
    assert len(nm) == len(kept) and max(nm) == point.Kr > point.K and sum(1 for x in nm if x > point.K) >= 20


def test_refusals(files):
    out = files["dir"] / "refused.sam"
    base = ("search", "-q", files["reads"], "-i", files["index"], "-o", out, "-e", K)
    rc, _, err = run(*base, *FRAG, "--sam")
    assert rc == 1 and "--sam needs --paired --best-pairs" in err and not out.exists()
    rc, _, err = run(*base, "--sam")
    assert rc == 1 and "--sam needs --paired --best-pairs" in err and not out.exists()
    rc, _, err = run(*base, *FRAG, "--best-pairs", "--sam", "--max_hits", 3)
    assert rc == 1 and "--sam cannot go with --max_hits" in err and not out.exists()
