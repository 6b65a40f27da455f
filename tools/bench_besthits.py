#!/usr/bin/env python3
"""besthits end to end, host queries to host hits, on one device.

100 Mbp single-record dna5 reference (sahara_synth_reference), 2M reads of
100 bp, one third each with 0, 1 and 2 errors (sahara_synth_reads_typed),
schemes h2-k2 with j = 0..2. Timed, best of 5 after one warm-up:

  a  search_best on the interleaved ranks (one rank per byte)
  b  search_best_packed_compact, codes in page-locked memory
  c  all-mode search_packed_compact with the (0, 2) scheme, for context

Each step runs in a process of its own under `timeout`, and prints one JSON
line. --lib selects another build of the library (SAHARA_HIP_LIB), e.g. the
parent commit's for the A/B; a step whose symbol that build lacks is skipped.

    python tools/bench_besthits.py [--lib PATH] [--steps a,b,c] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN, N_READS, READ_LEN, K = 100_000_000, 2_000_000, 100, 2
SPANS = ("seed_ms", "search_ms", "text_ms", "locate_ms", "sort_ms", "stage_ms", "output_ms")


def step(name, runs):
    sys.path.insert(0, ROOT)
    import numpy as np

    import sahara_amd as sa

    L = sa.lib()
    need = {"a": "sahara_gpu_search_best", "b": "sahara_gpu_search_best_packed_compact",
            "c": "sahara_gpu_search_packed_compact"}[name]
    if not hasattr(L, need):
        print(json.dumps({"step": name, "skipped": f"{need} missing in {sa.library_path()}"}))
        return
    flat, lens = sa.synth_reference([REF_LEN], sigma=6, seed=42)
    third = N_READS // 3
    reads = np.concatenate([sa.synth_reads(flat, lens, N_READS - 2 * third if e == 0 else third, READ_LEN, e, sigma=6,
                                           seed=7 + e) for e in range(K + 1)])
    reads = np.ascontiguousarray(reads[np.random.default_rng(1).permutation(len(reads))])
    idx = sa.BiFMIndex.build_flat(flat, lens, sigma=6)
    best = [sa.search_scheme("h2-k2", j, j, READ_LEN) for j in range(K + 1)]
    if name == "a":
        pats = sa.interleave_rc(reads, 6)
        call = lambda: len(sa.search_best(idx, pats, best))
    else:
        packed = sa.pack_reads(reads, 6, pinned=True)
        idx.prepare(2 * len(reads), READ_LEN)
        if name == "b":
            fn, arg = sa.search_best_packed_compact, best
        else:
            fn, arg = sa.search_packed_compact, sa.search_scheme("h2-k2", 0, K, READ_LEN)

        def call():
            c = fn(idx, packed, arg)
            n = len(c)
            c.close()
            return n
    times, hits, st = [], 0, {}
    for i in range(runs + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        hits = call()
        dt = time.perf_counter() - t0
        if i:
            times.append(dt)
        if i == 0 or dt <= min(times):
            st = idx.stats()
    best_s = min(times)
    print(json.dumps({"step": name, "build_id": sa.build_id(), "library": sa.library_path(), "reads": len(reads),
                      "patterns": 2 * len(reads), "read_len": READ_LEN, "hits": hits,
                      "seconds": [round(t, 4) for t in times], "best_s": round(best_s, 4),
                      "spread": round((max(times) - best_s) / best_s, 4),
                      "reads_per_s": round(len(reads) / best_s), "best_rounds": st.get("best_rounds", 0),
                      "batches": st["batches"], **{k: round(st[k], 3) for k in SPANS}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--steps", default="a,b,c")
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
