"""The planted case of the loci tests: a text in which one read maps to
several places (copies of a segment, two of them 157 apart, two in another
record), to long chains (tandem runs, a homopolymer) and to nothing, with the
CPU oracle's all-mode rows. No GPU: tests/test_loci_gpu.py runs it on one."""
import functools

import numpy as np

import oracle as O
import sahara_amd as sa
from helpers import acgt, hits_as_rows, mutate_reads

SIGMA, M, K = 6, 50, 2
# The seed is chosen so that the properties tests/test_loci_gpu.py asserts on the oracle's
# rows hold (seven different locus counts for W = 0..6, at most 2M hits, ...): with this
# builder 22 gives 228,184 hits and 4,196 / 1,086 / 819 / 800 / 683 / 534 / 518 loci; most
# other seeds draw an exact homopolymer read, whose ~770,000 rows take the total past 2M.
SEED = 22


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(SEED)
    A = acgt(SIGMA)
    r0 = A[rng.integers(0, 4, size=6000)]
    r1 = A[rng.integers(0, 4, size=3000)]
    seg = A[rng.integers(0, 4, size=120)]
    for at in (0, 500, 2500, 2657):
        r0[at:at + 120] = seg
    r1[1000:1120] = seg
    r1[-120:] = seg
    tandem = []
    for unit, at in ((3, 1000), (5, 1400), (6, 1800)):
        r0[at:at + 150] = np.resize(A[rng.integers(0, 4, size=unit)], 150)
        tandem.append(r0[at:at + 150].copy())
    r1[2000:2200] = A[rng.integers(0, 4)]
    homo = r1[2000:2200].copy()
    recs = [r0.astype(np.uint8), r1.astype(np.uint8)]
    parts = [mutate_reads(rng, [seg], 20, M, e, SIGMA) for e in range(3)]
    parts += [mutate_reads(rng, [t], 8, M, 1, SIGMA) for t in tandem]
    parts.append(mutate_reads(rng, [homo], 4, M, 1, SIGMA))
    parts.append(mutate_reads(rng, recs, 100, M, 2, SIGMA))
    parts.append(A[rng.integers(0, 4, size=(20, M))])
    reads = np.concatenate(parts).astype(np.uint8)
    reads = np.ascontiguousarray(reads[rng.permutation(len(reads))])
    pats = sa.interleave_rc(reads, SIGMA)
    scheme = sa.search_scheme("h2-k2", 0, K, M)
    ref = O.Index.build(recs, SIGMA, 16)
    want = hits_as_rows(ref.search(pats, scheme, edit=True, nthreads=8)[0])
    return dict(sigma=SIGMA, recs=recs, reads=reads, pats=pats, scheme=scheme, ref=ref, want=want)
