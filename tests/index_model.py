"""Python model of the bidirectional FM-index (index_build.hip, oracle/oracle.cpp).

Test infrastructure: `model()` states from the definitions, with Python's
bytes order and a naive sort, what both the GPU build and the CPU restatement
compute by prefix doubling — the text, both suffix arrays' BWTs, the C array,
the sampled-row bit words and the samples — so that the two implementations
are held to something that shares no algorithm with either. A proper prefix
sorts before its extensions in Python's bytes order, which is the convention
of kInitKeys / kPairKeys (a suffix that ends is smaller) and of the oracle.
tests/test_index_model.py holds the oracle to it without a GPU,
tests/test_index_edges.py the device build and the device load.
"""
import numpy as np


def text_of(records):
    """The records concatenated with a 0 ('$') after each; empty records allowed."""
    out = bytearray()
    for r in records:
        out += bytes(int(x) for x in r)
        out.append(0)
    return bytes(out)


def suffix_array(T):
    return sorted(range(len(T)), key=lambda i: T[i:])


def bwt_of(T, sa):
    n = len(T)
    return [T[(p - 1) % n] for p in sa]


def model(records, sigma, rate):
    """dict with n, n_records, rec_lens, text, sa, bwt_f, bwt_r, C (sigma + 1
    entries), sampled (n // 64 + 1 words), samples (row order), n_samples."""
    recs = [[int(x) for x in r] for r in records]
    assert rate >= 1 and all(1 <= x < sigma for r in recs for x in r)
    T = text_of(recs)
    R = text_of([r[::-1] for r in recs])
    n = len(T)
    sa = suffix_array(T)
    # in-record offset of every text position, and whether it is the delimiter
    off, delim = [], []
    for r in recs:
        off += list(range(len(r) + 1))
        delim += [False] * len(r) + [True]
    words = [0] * (n // 64 + 1)
    samples = []
    for row, p in enumerate(sa):
        if off[p] % rate == 0 or delim[p]:
            words[row // 64] |= 1 << (row % 64)
            samples.append(p)
    return dict(
        n=n, n_records=len(recs), rec_lens=np.array([len(r) for r in recs], np.uint64),
        text=np.frombuffer(T, np.uint8), sa=np.array(sa, np.uint32),
        bwt_f=np.array(bwt_of(T, sa), np.uint8), bwt_r=np.array(bwt_of(R, suffix_array(R)), np.uint8),
        C=np.array([sum(1 for x in T if x < c) for c in range(sigma + 1)], np.uint64),
        sampled=np.array(words, np.uint64), samples=np.array(samples, np.uint32), n_samples=len(samples))
