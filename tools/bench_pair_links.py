#!/usr/bin/env python3
"""The pair stage's links end to end, host reads to host hits and links, on one device.

The workload is tools/bench_pairs.py's and tools/bench_best_pairs.py's: a
100 Mbp single-record dna5 reference, 1M mate pairs of 100 bp reads with
fragments in [200, 500], a third of the pairs each with 0, 1 and 2
substitutions per mate; scheme h2-k2 (0, 2), all-mode, search_packed_compact
from pinned 2-bit reads. Timed, best of 5 after one warm-up, all runs listed:

  d  pairs and best pairs (delta 0), links off         (tools/bench_best_pairs.py's d)
  l  ... links on, and the links fetched (pair_links())
  e  loci (W = 2), pairs and best pairs, links off     (bench_best_pairs.py's e)
  m  ... links on, and the links fetched
  t  `sahara search --paired --best-pairs --emit-errors` end to end, index and reads from files
  s  `sahara search --paired --best-pairs --sam` end to end

Steps d, l, e, m share one process, one index and one set of reads, under
`timeout`. Each prints one JSON line: hits out, the bytes that crossed to the
host (records, summaries, links), the search call (with links: and their
fetch), its spread over the runs, the pair stage's kernel_ms
(sahara_gpu_pairs_stats: it includes the link kernels) and the link kernels'
own (sahara_gpu_pair_links_stats). --lib selects another build of the library
(SAHARA_HIP_LIB): a build without links runs d and e, which is how "links off
costs what the parent costs" is measured: the gap against the larger spread.
Steps t and s write the workload into --dir as an .idx and a FASTA file once
and time the command, best of --runs.

    python tools/bench_pair_links.py [--lib PATH] [--steps d,l,e,m] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_pairs import K, MAX_FRAGMENT, MIN_FRAGMENT, READ_LEN, SPANS, WINDOW, workload  # noqa: E402

# name: (loci, links)
STEPS = {"d": (False, False), "l": (False, True), "e": (True, False), "m": (True, True)}
CLI = {"t": ("--emit-errors",), "s": ("--sam",)}


def timed(call, runs, after):
    """bench_pairs.timed with the seconds to the microsecond: the links-off steps are compared
    with another build's to within their spread, which is a few tenths of a percent."""
    times, keep, out = [], {}, None
    for i in range(runs + 1):  # (the first is the warm-up)
        t0 = time.perf_counter()
        out = call()
        dt = time.perf_counter() - t0
        if i:
            times.append(dt)
        if i == 0 or dt <= min(times):
            keep = after()
    best = min(times)
    return out, dict(seconds=[round(t, 6) for t in times], best_s=round(best, 6),
                     spread=round((max(times) - best) / best, 4), **keep)


def steps(names, runs, workdir):
    sys.path.insert(0, ROOT)
    import numpy as np
    import sahara_amd as sa

    has = hasattr(sa.lib(), "sahara_gpu_set_pair_links")
    reads, idx = workload(sa)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    scheme = sa.search_scheme("h2-k2", 0, K, READ_LEN)
    for name in (n for n in names if n in STEPS):
        loci_on, links = STEPS[name]
        if links and not has:
            print(json.dumps({"step": name, "skipped": f"sahara_gpu_set_pair_links missing in {sa.library_path()}"}),
                  flush=True)
            continue
        idx.set_loci(WINDOW if loci_on else None)
        idx.set_pairs(MIN_FRAGMENT, MAX_FRAGMENT)
        idx.set_best_pairs(0)
        if has:
            idx.set_pair_links(links)

        def call():
            c = sa.search_packed_compact(idx, packed, scheme)
            n = len(c)
            c.close()
            if links:
                assert len(idx.pair_links()) == n
            return n

        def after():
            st, ps = idx.stats(), idx.pairs_stats()
            ls = idx.pair_links_stats() if has else {}
            return dict(batches=st["batches"], **{k: round(st[k], 3) for k in SPANS},
                        pairs_hits_in=ps["hits_in"], pairs_kept=ps["kept"], pairs=ps["pairs"],
                        pairs_kernel_ms=round(ps["kernel_ms"], 3), links=ls.get("links", 0),
                        primaries=ls.get("primaries", 0), links_kernel_ms=round(ls.get("kernel_ms", 0.0), 3))

        hits, fig = timed(call, runs, after)
        print(json.dumps({"step": name, "build_id": sa.build_id(), "library": sa.library_path(), "reads": len(reads),
                          "read_len": READ_LEN, "fragments": [MIN_FRAGMENT, MAX_FRAGMENT],
                          "window": WINDOW if loci_on else None, "pair_links": links, "hits": hits,
                          "download_bytes": 8 * hits + 8 * (len(reads) // 2) + (8 * hits if links else 0),
                          "reads_per_s": round(len(reads) / fig["best_s"]), **fig}), flush=True)
    cli = [n for n in names if n in CLI]
    if not cli:
        return
    os.makedirs(workdir, exist_ok=True)
    index, fasta = os.path.join(workdir, "ref.idx"), os.path.join(workdir, "reads.fa")
    idx.save(index)
    idx.close()
    letters = np.frombuffer(b"$ACGNT", np.uint8)
    with open(fasta, "wb") as f:
        for lo in range(0, len(reads), 1 << 16):
            block = letters[reads[lo:lo + (1 << 16)]]
            f.write(b"".join(b">r\n" + row.tobytes() + b"\n" for row in block))
    for name in cli:
        out = os.path.join(workdir, "out." + name)
        cmd = [os.path.join(ROOT, "bin", "sahara"), "search", "-q", fasta, "-i", index, "-o", out, "-e", str(K), "--paired",
               "--min-fragment", str(MIN_FRAGMENT), "--max-fragment", str(MAX_FRAGMENT), "--best-pairs", *CLI[name]]
        times, so = [], ""
        for _ in range(runs):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            times.append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"{' '.join(cmd)}: status {p.returncode}: {p.stderr[-2000:]}")
            so = p.stdout
        keep = [ln.strip() for ln in so.splitlines() if any(k in ln for k in (" time:", "number of hits", "pair links:",
                                                                               "best pairs:"))]
        print(json.dumps({"step": name, "command": " ".join(cmd[1:]), "seconds": [round(t, 3) for t in times],
                          "best_s": round(min(times), 3), "output_bytes": os.path.getsize(out), "stats": keep}), flush=True)
        os.remove(out)
    os.remove(index)
    os.remove(fasta)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--steps", default="d,l,e,m")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=500, help="seconds for the whole run")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--dir", default="/tmp/sahara_bench_pair_links", help="where steps t and s put their files")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)  # (run the steps here)
    a = ap.parse_args()
    names = a.steps.split(",")
    if a.child:
        return steps(names, a.runs, a.dir)
    env = dict(os.environ)
    if a.lib:
        env["SAHARA_HIP_LIB"] = os.path.abspath(a.lib)
    p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
                        "--steps", a.steps, "--runs", str(a.runs), "--dir", a.dir], env=env, stdout=subprocess.PIPE,
                       text=True)
    sys.stdout.write(p.stdout)
    if a.out and p.stdout:
        with open(a.out, "a") as f:
            f.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"the run ended with status {p.returncode}")


if __name__ == "__main__":
    main()
