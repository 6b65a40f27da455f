#!/usr/bin/env python3
"""Alignment of located hits, host records in to host records out, on one device.

tools/bench_besthits.py's shape: 100 Mbp single-record dna5 reference
(sahara_synth_reference), 2M reads of 100 bp, one third each with 0, 1 and 2
errors (sahara_synth_reads_typed), all-mode search_packed_compact with the
h2-k2 (0, 2) scheme, codes in page-locked memory; then align_packed_compact
(edit on, max_err 2) on the records of that search. Both calls are timed in
every run, best of 5 after one warm-up, runs listed. Reported: the alignment
call's ns per hit and hits per second, the kernel's own time (HIP events,
sahara_gpu_align_stats), the ratio of the alignment call to the search call
that produced the hits, and for scale the rate of the host-only Python model
(tests/align_model.py) on a sample of the same hits, one thread.

The run is a process of its own under `timeout` and prints one JSON line.

    python tools/bench_align.py [--runs N] [--sample N] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN, N_READS, READ_LEN, K = 100_000_000, 2_000_000, 100, 2


def step(runs, sample):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import align_model as am
    import sahara_amd as sa

    flat, lens = sa.synth_reference([REF_LEN], sigma=6, seed=42)
    third = N_READS // 3
    reads = np.concatenate([sa.synth_reads(flat, lens, N_READS - 2 * third if e == 0 else third, READ_LEN, e, sigma=6,
                                           seed=7 + e) for e in range(K + 1)])
    reads = np.ascontiguousarray(reads[np.random.default_rng(1).permutation(len(reads))])
    idx = sa.BiFMIndex.build_flat(flat, lens, sigma=6)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    sch = sa.search_scheme("h2-k2", 0, K, READ_LEN)
    search_s, align_s, kernel_ms, stage_ms = [], [], [], []
    hits = none = 0
    sampled = None
    for i in range(runs + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        c = sa.search_packed_compact(idx, packed, sch)
        t1 = time.perf_counter()
        recs = sa.align_packed_compact(idx, packed, c, edit=True, max_err=K)
        t2 = time.perf_counter()
        st = sa.align_stats(idx)
        hits = len(c)
        none = int((recs["err"] == sa.ALIGN_NONE).sum())
        if i:
            search_s.append(t1 - t0)
            align_s.append(t2 - t1)
            kernel_ms.append(st["kernel_ms"])
            stage_ms.append(st["stage_ms"])
        if i == runs and sample:  # the model's rate on a sample of these hits, and a check of the records
            pick = np.random.default_rng(2).integers(0, hits, size=sample)
            h = c.to_hits()[pick]
            sampled = (h, recs[pick].copy())
        c.close()
        del recs
    out = {"build_id": sa.build_id(), "reads": len(reads), "patterns": 2 * len(reads), "read_len": READ_LEN,
           "max_err": K, "hits": hits, "none": none,
           "search_s": [round(t, 4) for t in search_s], "align_s": [round(t, 4) for t in align_s],
           "kernel_ms": [round(t, 3) for t in kernel_ms], "stage_ms": [round(t, 3) for t in stage_ms]}
    a, s, k = min(align_s), min(search_s), min(kernel_ms)
    out.update({"align_best_s": round(a, 4), "align_spread": round((max(align_s) - a) / a, 4),
                "search_best_s": round(s, 4), "search_spread": round((max(search_s) - s) / s, 4),
                "ns_per_hit": round(a / hits * 1e9, 3), "hits_per_s": round(hits / a),
                "kernel_best_ms": round(k, 3), "kernel_spread": round((max(kernel_ms) - k) / k, 4),
                "kernel_ns_per_hit": round(k * 1e6 / hits, 4),
                "align_over_search": round(a / s, 3), "kernel_over_search": round(k / 1e3 / s, 4)})
    if sampled:
        h, got = sampled
        pats = sa.interleave_rc(reads, 6)
        T = np.append(flat, np.uint8(0))
        t0 = time.perf_counter()
        want = [am.record_of(am.align(pats[int(x["qid"])].tolist(), T, int(x["pos"]), K, True)) for x in h]
        dt = time.perf_counter() - t0
        same = all((int(r["err"]), int(r["ref_len"]), r["edit"].tolist()) == w for r, w in zip(got, want))
        out.update({"model_sample": len(h), "model_hits_per_s": round(len(h) / dt), "model_equal": bool(same)})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000, help="hits the Python model aligns (0: none)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds")
    ap.add_argument("--out", help="append the JSON line to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return step(a.runs, a.sample)
    p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
                        "--runs", str(a.runs), "--sample", str(a.sample)], stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if a.out and p.stdout:
        with open(a.out, "a") as f:
            f.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"the run ended with status {p.returncode}")


if __name__ == "__main__":
    main()
