#!/usr/bin/env python3
"""The mate rescue end to end, host reads to host hits, on one device.

100 Mbp single-record dna5 reference (sahara_synth_reference), 2M reads of
100 bp taken as 1M mate pairs: mate A from [a, a + 100), mate B the reverse
complement of [a + F - 100, a + F) with F drawn in [100, 500]; both mates
carry p % 3 substitutions, and mate B of every tenth pair carries 4 to 6
instead, which `-e 2` does not find. Scheme h2-k2 (0, 2), all-mode,
search_packed_compact from pinned 2-bit reads, pairs on with fragments
[0, 500]. Timed, best of 5 after one warm-up, all runs listed:

  a  rescue off (the call as the parent commit runs it: --lib takes that build)
  r  rescue 6, the default cap of 64 anchors
  l  loci on (W = 2), rescue off
  s  loci on, rescue 6
  e  the alternative the rescue replaces: `-e 6` for every read (h2-k2 (0, 6)), loci on with W = 6 so
     that the output stays comparable, on --e6-pairs pairs (all of them take minutes and 10^10 rows)

Each step runs in a process of its own under `timeout`, and prints one JSON
line: hits out, the pairs with a kept hit, the share of the noisy pairs among
them, the search call, and the stages' figures (sahara_gpu_rescue_stats,
sahara_gpu_pairs_stats, sahara_gpu_loci_stats). --lib selects another build of
the library (SAHARA_HIP_LIB); a step that build cannot run is skipped.

    python tools/bench_rescue.py [--lib PATH [--label NAME]] [--steps a,r,l,s,e] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN, N_PAIRS, READ_LEN, K, WINDOW = 100_000_000, 1_000_000, 100, 2, 2
MIN_FRAGMENT, MAX_FRAGMENT = 0, 500
RESCUE, NOISY_EVERY = 6, 10
SPANS = ("seed_ms", "search_ms", "text_ms", "locate_ms", "sort_ms", "stage_ms", "output_ms")
STEPS = {  # name: (rescue, loci window or None, the search's k)
    "a": (0, None, K), "r": (RESCUE, None, K), "l": (0, WINDOW, K), "s": (RESCUE, WINDOW, K), "e": (0, RESCUE, RESCUE),
}


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


def workload(sa, n_pairs):
    import numpy as np
    flat, lens = sa.synth_reference([REF_LEN], sigma=6, seed=42)
    text = np.asarray(flat[:REF_LEN])
    rng = np.random.default_rng(1)
    a = rng.integers(0, REF_LEN - MAX_FRAGMENT, size=n_pairs)
    frag = rng.integers(READ_LEN, MAX_FRAGMENT + 1, size=n_pairs)
    col = np.arange(READ_LEN)
    mate_a = text[a[:, None] + col]
    comp = np.array([0, 5, 3, 2, 4, 1], np.uint8)  # dna5 ranks: $ A C G N T
    mate_b = comp[text[(a + frag - 1)[:, None] - col]]
    reads = np.empty((2 * n_pairs, READ_LEN), np.uint8)
    reads[0::2], reads[1::2] = mate_a, mate_b
    acgt = np.array([1, 2, 3, 5], np.uint8)
    pair = np.arange(n_pairs)
    errs = np.repeat(pair % (K + 1), 2)  # both mates of pair p get p % 3 substitutions ...
    noisy = pair % NOISY_EVERY == 0
    errs[1::2][noisy] = 4 + (pair[noisy] // NOISY_EVERY) % 3  # ... and mate B of every tenth pair 4 to 6
    for e in range(1, int(errs.max()) + 1):
        rows = np.flatnonzero(errs >= e)
        at = rng.integers(0, READ_LEN, size=len(rows))  # (two of a read's may meet: it then has one fewer)
        reads[rows, at] = acgt[(np.searchsorted(acgt, reads[rows, at]) + rng.integers(1, 4, size=len(rows))) % 4]
    idx = sa.BiFMIndex.build_flat(flat, lens, sigma=6)
    return np.ascontiguousarray(reads), idx, noisy


def library_label(sa):
    """--label's name for the library, else its path relative to the repository (a build outside it: its
    file name alone)."""
    if os.environ.get("SAHARA_BENCH_LABEL"):
        return os.environ["SAHARA_BENCH_LABEL"]
    rel = os.path.relpath(os.path.realpath(sa.library_path()), os.path.realpath(ROOT))
    return os.path.basename(rel) if rel.startswith("..") else rel


def step(name, runs, e6_pairs):
    sys.path.insert(0, ROOT)
    import numpy as np

    import sahara_amd as sa

    rescue, window, k = STEPS[name]
    has = hasattr(sa.lib(), "sahara_gpu_set_rescue")
    if rescue and not has:
        print(json.dumps({"step": name, "skipped": f"sahara_gpu_set_rescue missing in {library_label(sa)}"}))
        return
    n_pairs = e6_pairs if name == "e" else N_PAIRS
    reads, idx, noisy = workload(sa, n_pairs)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    scheme = sa.search_scheme("h2-k2", 0, k, READ_LEN)
    if window is not None:
        idx.set_loci(window)
    idx.set_pairs(MIN_FRAGMENT, MAX_FRAGMENT)
    if rescue:
        idx.set_rescue(rescue)
    found = {}

    def call():
        c = sa.search_packed_compact(idx, packed, scheme)
        n = len(c)
        if not found:  # (the warm-up run: which pairs came back)
            pairs = np.unique(c.to_hits()["qid"] >> np.uint64(2)).astype(np.int64)
            found.update(pairs=len(pairs), noisy_pairs=int(noisy[pairs].sum()))
        c.close()
        return n

    def after():
        st = idx.stats()
        ls = idx.loci_stats()
        ps = idx.pairs_stats()
        rs = idx.rescue_stats() if has else dict(anchors=0, capped_queries=0, starts=0, rescued=0, batches=0, kernel_ms=0.0)
        return dict(batches=st["batches"], **{k: round(st[k], 3) for k in SPANS},
                    loci=ls["loci"], loci_kernel_ms=round(ls["kernel_ms"], 3),
                    pairs_hits_in=ps["hits_in"], pairs_kept=ps["kept"], pairs_kernel_ms=round(ps["kernel_ms"], 3),
                    anchors=rs["anchors"], capped_queries=rs["capped_queries"], starts=rs["starts"],
                    rescued=rs["rescued"], rescue_kernel_ms=round(rs["kernel_ms"], 3))

    hits, fig = timed(call, runs, after)
    print(json.dumps({"step": name, "build_id": sa.build_id(), "library": library_label(sa), "reads": len(reads),
                      "read_len": READ_LEN, "errors": k, "fragments": [MIN_FRAGMENT, MAX_FRAGMENT], "rescue": rescue or None,
                      "window": window, "hits": hits, "pairs_found": found["pairs"],
                      "noisy_pairs": int(noisy.sum()), "noisy_pairs_found": found["noisy_pairs"],
                      "reads_per_s": round(len(reads) / fig["best_s"]), **fig}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--label", help="what the JSON lines call the library (--lib parent.so --label parent)")
    ap.add_argument("--steps", default="a,r,l,s,e")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--e6-pairs", type=int, default=2_000, help="pairs of step e")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--step", help=argparse.SUPPRESS)  # (a child: run one step here)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.runs, a.e6_pairs)
    env = dict(os.environ)
    if a.lib:
        env["SAHARA_HIP_LIB"] = os.path.abspath(a.lib)
    if a.label:
        env["SAHARA_BENCH_LABEL"] = a.label
    for s in a.steps.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", s,
                            "--runs", str(a.runs), "--e6-pairs", str(a.e6_pairs)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        sys.stderr.write(p.stderr)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if a.out and p.stdout:
            with open(a.out, "a") as f:
                f.write(p.stdout)
        if p.returncode != 0:  # a step that failed or ran out of time ends the run, and is recorded
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps({"step": s, "e6_pairs": a.e6_pairs if s == "e" else None, "status": p.returncode,
                                        "error": p.stderr.strip().splitlines()[-1:]}) + "\n")
            sys.exit(f"step {s} ended with status {p.returncode}")


if __name__ == "__main__":
    main()
