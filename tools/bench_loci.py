#!/usr/bin/env python3
"""The loci stage end to end, host reads to host hits, on one device.

100 Mbp single-record dna5 reference (sahara_synth_reference), 2M reads of
100 bp, one third each with 0, 1 and 2 errors (sahara_synth_reads_typed),
scheme h2-k2 (0, 2), all-mode: the workload of tools/bench_besthits.py.
Timed, best of 5 after one warm-up:

  a  search_packed_compact, loci off
  b  search_packed_compact, loci on with W = 2
  c  a, then align_packed_compact on its records
  d  b, then align_packed_compact on its records
  q  the stage's shape on a query inside a repeat: the planted case of
     tests/loci_case.py in one batch (its largest query has ~30,000 rows),
     loci W = 0 (one thread per hit) against --max_hits 2^32 - 1, which
     returns the same rows through limitBatch (one thread per query)

Each step runs in a process of its own under `timeout`, and prints one JSON
line: hits out, the bytes of the records that crossed to the host, the
stage's figures (sahara_gpu_loci_stats). --lib selects another build of the
library (SAHARA_HIP_LIB); a step that build cannot run is skipped.

    python tools/bench_loci.py [--lib PATH] [--steps a,b,c,d,q] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN, N_READS, READ_LEN, K, WINDOW = 100_000_000, 2_000_000, 100, 2, 2
SPANS = ("seed_ms", "search_ms", "text_ms", "locate_ms", "sort_ms", "stage_ms", "output_ms")


def timed(call, runs, after):
    """call() runs + 1 times (the first is the warm-up); after() once per run
    gives the figures kept from the fastest."""
    times, keep, out = [], {}, None
    for i in range(runs + 1):
        t0 = time.perf_counter()
        out = call()
        dt = time.perf_counter() - t0
        if i:
            times.append(dt)
        if i == 0 or dt <= min(times):
            keep = after()
    best = min(times)
    return out, dict(seconds=[round(t, 4) for t in times], best_s=round(best, 4),
                     spread=round((max(times) - best) / best, 4), **keep)


def workload(sa):
    import numpy as np
    flat, lens = sa.synth_reference([REF_LEN], sigma=6, seed=42)
    third = N_READS // 3
    reads = np.concatenate([sa.synth_reads(flat, lens, N_READS - 2 * third if e == 0 else third, READ_LEN, e, sigma=6,
                                           seed=7 + e) for e in range(K + 1)])
    reads = np.ascontiguousarray(reads[np.random.default_rng(1).permutation(len(reads))])
    idx = sa.BiFMIndex.build_flat(flat, lens, sigma=6)
    return reads, idx


def step(name, runs):
    sys.path.insert(0, ROOT)
    import sahara_amd as sa

    has_loci = hasattr(sa.lib(), "sahara_gpu_set_loci")
    if name in "bdq" and not has_loci:
        print(json.dumps({"step": name, "skipped": f"sahara_gpu_set_loci missing in {sa.library_path()}"}))
        return
    head = {"step": name, "build_id": sa.build_id(), "library": sa.library_path()}
    if name == "q":
        return step_query(sa, head, runs)
    reads, idx = workload(sa)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    scheme = sa.search_scheme("h2-k2", 0, K, READ_LEN)
    loci_on, with_align = name in "bd", name in "cd"
    if loci_on:
        idx.set_loci(WINDOW)
    split = {}

    def call():
        t0 = time.perf_counter()
        c = sa.search_packed_compact(idx, packed, scheme)
        split["search_s"] = round(time.perf_counter() - t0, 4)
        n = len(c)
        if with_align:
            t1 = time.perf_counter()
            sa.align_packed_compact(idx, packed, c, max_err=K)
            split["align_s"] = round(time.perf_counter() - t1, 4)
            split["align_kernel_ms"] = round(sa.align_stats(idx)["kernel_ms"], 3)
        c.close()
        return n

    def after():
        st = idx.stats()
        ls = idx.loci_stats() if has_loci else dict(hits_in=0, loci=0, batches=0, kernel_ms=0.0)
        return dict(split, batches=st["batches"], **{k: round(st[k], 3) for k in SPANS},
                    loci_hits_in=ls["hits_in"], loci=ls["loci"], loci_batches=ls["batches"],
                    loci_kernel_ms=round(ls["kernel_ms"], 3))

    hits, fig = timed(call, runs, after)
    print(json.dumps({**head, "reads": len(reads), "patterns": 2 * len(reads), "read_len": READ_LEN,
                      "window": WINDOW if loci_on else None, "align": with_align, "hits": hits,
                      "download_bytes": 8 * hits, "reads_per_s": round(len(reads) / fig["best_s"]), **fig}))


def step_query(sa, head, runs):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    from loci_case import SIGMA, planted
    c = planted()
    rows = c["want"]
    idx = sa.BiFMIndex.build(c["recs"], sigma=SIGMA)
    largest = int(np.unique(rows[:, 0], return_counts=True)[1].max())
    out = {**head, "rows": len(rows), "largest_query_rows": largest, "patterns": len(c["pats"])}
    plain = lambda: dict(sort_ms=round(idx.stats()["sort_ms"], 4))
    _, f = timed(lambda: len(sa.search(idx, c["pats"], c["scheme"])), runs, plain)
    out["off"] = f
    n_lim, f = timed(lambda: len(sa.search(idx, c["pats"], c["scheme"], max_hits=0xFFFFFFFF)), runs, plain)
    out["per_query_limit"] = dict(f, hits=n_lim)
    idx.set_loci(0)
    n_loci, f = timed(lambda: len(sa.search(idx, c["pats"], c["scheme"])), runs,
                      lambda: dict(sort_ms=round(idx.stats()["sort_ms"], 4),
                                   loci_kernel_ms=round(idx.loci_stats()["kernel_ms"], 4)))
    out["per_hit_loci"] = dict(f, hits=n_loci)
    assert n_lim == n_loci, (n_lim, n_loci)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--steps", default="a,b,c,d,q")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--step", help=argparse.SUPPRESS)  # (a child: run one step here)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.runs)
    env = dict(os.environ)
    if a.lib:
        env["SAHARA_HIP_LIB"] = os.path.abspath(a.lib)
    for s in a.steps.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", s,
                            "--runs", str(a.runs)], env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if a.out and p.stdout:
            with open(a.out, "a") as f:
                f.write(p.stdout)
        if p.returncode != 0:  # a step that failed or ran out of time ends the run
            sys.exit(f"step {s} ended with status {p.returncode}")


if __name__ == "__main__":
    main()
