"""The command line's writers (sahara_amd/cli/output.h: writeSam, writeHits)
on the CPU: tests/cli_output_check.cpp, built alone under the address and
undefined-behaviour sanitizers, writes the planted case of
tests/pair_links_case.py (the model's kept rows and links, tests/align_model.py's
alignments, the reads as 2-bit codes with an N list) as one shard, as two cut
at a pair border, as three of which the middle one has no hit and as two of
which the first has none, each shard's records over many blocks, with writer
blocks of 3 pairs and 5 hits and with 1 and 3 threads. Every file is
tests/sam_model.py's text, or the hit lines formatted here from the model's
rows, byte for byte: all layouts write the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import align_model as am
import sahara_amd as sa
from best_pairs_case import K, M, SIGMA, WIDE
from pair_links_case import check, expected_links
from sam_model import sam_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAM_BLOCK = 3  # pairs per writer block, as the program passes it
N_RANK = 4


def with_n(c, has_hit):
    """The case's reads with some N: in pairs that keep nothing (the first and
    the last symbol of a read, two in a row, the stream's first symbol if pair
    0 keeps nothing) and in both mates of the "clean" pair, whose two records
    then align with one substitution each (the second as a reverse complement)."""
    reads = c["reads"].copy()
    none = np.flatnonzero(~has_hit)
    assert len(none) >= 3
    reads[2 * none[0], 0] = N_RANK
    reads[2 * none[0] + 1, M - 1] = N_RANK
    reads[2 * none[1], 7:9] = N_RANK
    reads[2 * none[-1] + 1, [0, M - 1]] = N_RANK
    clean, = (e["pair"] for e in c["plan"] if e["kind"] == "clean")
    assert has_hit[clean]
    reads[2 * clean, 20] = N_RANK
    reads[2 * clean + 1, 30] = N_RANK
    return reads


def pack_reads(reads):
    """Two bits per symbol (A C G T = 0 1 2 3; an N's code is arbitrary: 0), and the N positions."""
    flat = reads.reshape(-1)
    code = np.array([0, 0, 1, 2, 0, 3], np.uint8)[flat]
    code = np.concatenate([code, np.zeros(-len(code) % 4, np.uint8)]).reshape(-1, 4)
    packed = (code[:, 0] | code[:, 1] << 2 | code[:, 2] << 4 | code[:, 3] << 6).astype(np.uint8)
    return packed, np.flatnonzero(flat == N_RANK).astype("<u8")


def layouts(has_hit):
    """Shard borders (in pairs) of the layouts: one shard; two, cut beside a
    pair that keeps nothing; three, the middle one a run of such pairs; and two
    of which the first is pair 0 alone, which keeps nothing."""
    n = len(has_hit)
    none = np.flatnonzero(~has_hit)
    inner = none[(none > 1) & (none < n - 1)]
    run = next(int(p) for p in inner if not has_hit[p + 1] and p + 2 < n)  # pairs run, run + 1 keep nothing
    assert not has_hit[0]
    return [[n], [int(inner[len(inner) // 3]), n], [run, run + 2, n], [1, n]], none


def test_writers_on_the_planted_case(tmp_path):
    c = check()
    kept, summary, links, info = expected_links(WIDE, 0)
    n_pairs = c["n_pairs"]
    has_hit = np.zeros(n_pairs, bool)
    has_hit[(kept[:, 0] >> np.uint64(2)).astype(np.int64)] = True
    cuts, none = layouts(has_hit)
    # the condition of the writer's border logic: in every layout a pair that keeps nothing lies in the middle
    # of a writer block (blocks count from each shard's first pair); with more than one shard, one lies at a
    # shard's border, on either side of it
    for lay in cuts:
        origins = np.array(sorted({0} | {a for a, b in zip([0] + lay[:-1], lay) if has_hit[a:b].any()}))
        offset = none - origins[np.searchsorted(origins, none, side="right") - 1]
        assert (offset % SAM_BLOCK == 1).any(), lay
        for b in lay[:-1]:
            assert not has_hit[b] or not has_hit[b - 1], lay
    assert not has_hit[cuts[2][0]:cuts[2][1]].any() and not has_hit[cuts[1][0]]

    reads = with_n(c, has_hit)
    pats = sa.interleave_rc(reads, SIGMA)
    assert (pats == N_RANK).sum() == 2 * (reads == N_RANK).sum() >= 16
    T = am.concat_text(c["recs"])
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in c["recs"]])]).astype("<u8")
    aligned = [am.align(pats[q].tolist(), T, int(starts[s]) + p, K, True) for q, s, p, e in kept.tolist()]
    assert all(a is not None for a in aligned) and sum(a[0] > 0 for a in aligned) > 100

    packed, npos = pack_reads(reads)
    rows = np.zeros(len(kept), np.dtype([("qid", "<u8"), ("seq", "<u4"), ("err", "<u4"), ("pos", "<u8")]))
    rows["qid"], rows["seq"], rows["pos"], rows["err"] = kept[:, 0], kept[:, 1], kept[:, 2], kept[:, 3]
    aln = np.zeros(len(kept), np.dtype([("err", "<u4"), ("ref_len", "<u4"), ("edit", "<u2", am.MAX_ERR)]))
    for i, a in enumerate(aligned):
        aln[i] = am.record_of(a)
    flat_cuts = np.array([p for lay in cuts for p in lay], "<u8")
    case = tmp_path / "case.bin"
    with open(case, "wb") as f:
        f.write(np.array([len(kept), n_pairs, M, len(c["recs"]), len(packed), len(npos), len(flat_cuts)], "<u8").tobytes())
        for a in (flat_cuts, starts, rows, links, aln, packed, npos):
            f.write(np.ascontiguousarray(a).tobytes())

    exe = tmp_path / "cli_output_check"
    lib = os.path.join(ROOT, "sahara_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libsahara_hip.so")):
        pytest.fail("libsahara_hip.so missing: run `make` (or __graft_entry__.build())")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cli_output_check.cpp"),
                    "-o", str(exe), "-L" + lib, "-lsahara_hip",
                    "-Wl,-rpath," + lib, "-lpthread"], check=True)
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([str(exe), str(case), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "" and p.stdout == "4 layouts\n", (p.returncode, p.stdout, p.stderr[-4000:])

    cigars = [am.cigar(a[2], M) for a in aligned]
    want = {
        "sam": sam_text(c["recs"], pats, SIGMA, kept, links, n_pairs, K),
        "plain": "".join(f"{q} {s} {p}\n" for q, s, p, e in kept.tolist()),
        "errors": "".join(f"{q} {s} {p} {e}\n" for q, s, p, e in kept.tolist()),
        "cigar": "".join(f"{q} {s} {p} {e} {cg}\n" for (q, s, p, e), cg in zip(kept.tolist(), cigars)),
    }
    want["whole"] = want["cigar"]  # the same lines from whole sahara_hit records
    assert "N" in want["sam"] and any("X" in cg for cg in cigars)
    names = sorted(os.listdir(out))
    assert names == sorted(f"{kind}_L{lay}_t{nt}" for kind in want for lay in range(len(cuts)) for nt in (1, 3))
    for name in names:
        assert (out / name).read_text() == want[name.split("_")[0]], name
