#!/usr/bin/env python3
"""The pair stage end to end, host reads to host hits, on one device.

100 Mbp single-record dna5 reference (sahara_synth_reference), 2M reads of
100 bp taken as 1M mate pairs: mate A from [a, a + 100), mate B the reverse
complement of [a + F - 100, a + F) with F drawn in [200, 500], the stage's
window; a third of the pairs each with 0, 1 and 2 substitutions per mate.
Scheme h2-k2 (0, 2), all-mode, search_packed_compact from pinned 2-bit reads.
Timed, best of 5 after one warm-up, all runs listed:

  a  pairs off
  b  pairs on, fragments [200, 500]
  l  loci on (W = 2), pairs off: the yardstick stage on the same hits
  c  loci and pairs on

Each step runs in a process of its own under `timeout`, and prints one JSON
line: hits out, the bytes of the records that crossed to the host, the search
call, sort_ms, and the stages' figures (sahara_gpu_pairs_stats,
sahara_gpu_loci_stats). --lib selects another build of the library
(SAHARA_HIP_LIB); a step that build cannot run is skipped.

    python tools/bench_pairs.py [--lib PATH] [--steps a,b,l,c] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN, N_PAIRS, READ_LEN, K, WINDOW = 100_000_000, 1_000_000, 100, 2, 2
MIN_FRAGMENT, MAX_FRAGMENT = 200, 500
SPANS = ("seed_ms", "search_ms", "text_ms", "locate_ms", "sort_ms", "stage_ms", "output_ms")
STEPS = {"a": (False, False), "b": (True, False), "l": (False, True), "c": (True, True)}  # name: (pairs, loci)


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
    text = np.asarray(flat[:REF_LEN])
    rng = np.random.default_rng(1)
    a = rng.integers(0, REF_LEN - MAX_FRAGMENT, size=N_PAIRS)
    frag = rng.integers(MIN_FRAGMENT, MAX_FRAGMENT + 1, size=N_PAIRS)
    col = np.arange(READ_LEN)
    mate_a = text[a[:, None] + col]
    comp = np.array([0, 5, 3, 2, 4, 1], np.uint8)  # dna5 ranks: $ A C G N T
    mate_b = comp[text[(a + frag - 1)[:, None] - col]]
    reads = np.empty((2 * N_PAIRS, READ_LEN), np.uint8)
    reads[0::2], reads[1::2] = mate_a, mate_b
    acgt = np.array([1, 2, 3, 5], np.uint8)
    errs = np.repeat(np.arange(N_PAIRS) % (K + 1), 2)  # both mates of pair p get p % 3 substitutions
    for e in range(1, K + 1):
        rows = np.flatnonzero(errs >= e)
        at = rng.integers(0, READ_LEN, size=len(rows))
        reads[rows, at] = acgt[(np.searchsorted(acgt, reads[rows, at]) + rng.integers(1, 4, size=len(rows))) % 4]
    idx = sa.BiFMIndex.build_flat(flat, lens, sigma=6)
    return np.ascontiguousarray(reads), idx


def step(name, runs):
    sys.path.insert(0, ROOT)
    import sahara_amd as sa

    pairs_on, loci_on = STEPS[name]
    has = hasattr(sa.lib(), "sahara_gpu_set_pairs")
    if pairs_on and not has:
        print(json.dumps({"step": name, "skipped": f"sahara_gpu_set_pairs missing in {sa.library_path()}"}))
        return
    reads, idx = workload(sa)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    scheme = sa.search_scheme("h2-k2", 0, K, READ_LEN)
    if loci_on:
        idx.set_loci(WINDOW)
    if pairs_on:
        idx.set_pairs(MIN_FRAGMENT, MAX_FRAGMENT)

    def call():
        c = sa.search_packed_compact(idx, packed, scheme)
        n = len(c)
        c.close()
        return n

    def after():
        st = idx.stats()
        ls = idx.loci_stats()
        ps = idx.pairs_stats() if has else dict(hits_in=0, kept=0, pairs=0, batches=0, kernel_ms=0.0)
        return dict(batches=st["batches"], **{k: round(st[k], 3) for k in SPANS},
                    loci_hits_in=ls["hits_in"], loci=ls["loci"], loci_kernel_ms=round(ls["kernel_ms"], 3),
                    pairs_hits_in=ps["hits_in"], pairs_kept=ps["kept"], pairs=ps["pairs"],
                    pairs_batches=ps["batches"], pairs_kernel_ms=round(ps["kernel_ms"], 3))

    hits, fig = timed(call, runs, after)
    print(json.dumps({"step": name, "build_id": sa.build_id(), "library": sa.library_path(), "reads": len(reads),
                      "patterns": 2 * len(reads), "read_len": READ_LEN,
                      "fragments": [MIN_FRAGMENT, MAX_FRAGMENT] if pairs_on else None,
                      "window": WINDOW if loci_on else None, "hits": hits, "download_bytes": 8 * hits,
                      "reads_per_s": round(len(reads) / fig["best_s"]), **fig}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--steps", default="a,b,l,c")
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
