#!/usr/bin/env python3
"""The pair stage's best mode end to end, host reads to host hits, on one device.

The workload is tools/bench_pairs.py's: a 100 Mbp single-record dna5
reference, 1M mate pairs of 100 bp reads with fragments in [200, 500], a third
of the pairs each with 0, 1 and 2 substitutions per mate; scheme h2-k2 (0, 2),
all-mode, search_packed_compact from pinned 2-bit reads. Timed, best of 5
after one warm-up, all runs listed:

  b  pairs on, fragments [200, 500]                    (the plain pair stage)
  d  ... and best pairs, delta 0
  c  loci (W = 2) and pairs on
  e  ... and best pairs, delta 0
  w  pairs on, fragments [200, 100000]                 (a deliberately wide window)
  x  ... and best pairs, delta 0

All steps of a run share one process, one index and one set of reads, under
`timeout`. Each prints one JSON line: hits out, the bytes of the records that
crossed to the host, the search call, the pair stage's kernel_ms
(sahara_gpu_pairs_stats; with best pairs on it includes the mode's kernels)
and the mode's figures (sahara_gpu_best_pairs_stats). --lib selects another
build of the library (SAHARA_HIP_LIB): a build without the mode runs b, c, w.

    python tools/bench_best_pairs.py [--lib PATH] [--steps b,d,c,e,w,x] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_pairs import K, MAX_FRAGMENT, MIN_FRAGMENT, READ_LEN, SPANS, WINDOW, timed, workload  # noqa: E402

WIDE_FRAGMENT = 100_000
# name: (loci, max_fragment, best)
STEPS = {"b": (False, MAX_FRAGMENT, False), "d": (False, MAX_FRAGMENT, True), "c": (True, MAX_FRAGMENT, False),
         "e": (True, MAX_FRAGMENT, True), "w": (False, WIDE_FRAGMENT, False), "x": (False, WIDE_FRAGMENT, True)}


def steps(names, runs):
    sys.path.insert(0, ROOT)
    import sahara_amd as sa

    has = hasattr(sa.lib(), "sahara_gpu_set_best_pairs")
    reads, idx = workload(sa)
    packed = sa.pack_reads(reads, 6, pinned=True)
    idx.prepare(2 * len(reads), READ_LEN)
    scheme = sa.search_scheme("h2-k2", 0, K, READ_LEN)
    for name in names:
        loci_on, max_fragment, best = STEPS[name]
        if best and not has:
            print(json.dumps({"step": name, "skipped": f"sahara_gpu_set_best_pairs missing in {sa.library_path()}"}),
                  flush=True)
            continue
        idx.set_loci(WINDOW if loci_on else None)
        idx.set_pairs(MIN_FRAGMENT, max_fragment)
        if has:
            idx.set_best_pairs(0 if best else None)

        def call():
            c = sa.search_packed_compact(idx, packed, scheme)
            n = len(c)
            c.close()
            return n

        def after():
            st, ps = idx.stats(), idx.pairs_stats()
            bs = idx.best_pairs_stats() if has else {}
            return dict(batches=st["batches"], **{k: round(st[k], 3) for k in SPANS},
                        pairs_hits_in=ps["hits_in"], pairs_kept=ps["kept"], pairs=ps["pairs"],
                        pairs_kernel_ms=round(ps["kernel_ms"], 3), best_kept=bs.get("kept", 0),
                        unique_pairs=bs.get("unique_pairs", 0))

        hits, fig = timed(call, runs, after)
        print(json.dumps({"step": name, "build_id": sa.build_id(), "library": sa.library_path(), "reads": len(reads),
                          "read_len": READ_LEN, "fragments": [MIN_FRAGMENT, max_fragment],
                          "window": WINDOW if loci_on else None, "best_pairs": best, "hits": hits,
                          "download_bytes": 8 * hits + (8 * (len(reads) // 2) if best else 0),
                          "reads_per_s": round(len(reads) / fig["best_s"]), **fig}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="another build of libsahara_hip.so (SAHARA_HIP_LIB)")
    ap.add_argument("--steps", default="b,d,c,e,w,x")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=500, help="seconds for the whole run")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)  # (run the steps here)
    a = ap.parse_args()
    names = a.steps.split(",")
    if a.child:
        return steps(names, a.runs)
    env = dict(os.environ)
    if a.lib:
        env["SAHARA_HIP_LIB"] = os.path.abspath(a.lib)
    p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
                        "--steps", a.steps, "--runs", str(a.runs)], env=env, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    if a.out and p.stdout:
        with open(a.out, "a") as f:
            f.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"the run ended with status {p.returncode}")


if __name__ == "__main__":
    main()
