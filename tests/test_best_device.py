"""besthits on the device: the exact-j schemes run as rounds inside each batch
of the streamed pass (pass.cpp issueFM), a round seeding only
the queries without a located row so far.

Expected everywhere: oracle.search_best over the interleaved patterns (with
test_golden's limit_rows where max_hits is given), compared as sorted rows,
bit-exact. 500 reads of 50 bp with 0..3 errors plus random ones over a
repeat-rich two-record text: exact reads inside repeats have many rows in
round 0, the 3-error and random reads survive every round (or are found by
luck)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import acgt, hits_as_rows, mutate_reads, random_records

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(sigma=6, with_n=False, gen="h2-k2", k=2, m=50, seed=5):
    """Text, reads, schemes and the oracle's results, computed once per shape."""
    rng = np.random.default_rng(seed)
    recs = random_records(rng, [25000, 8000], sigma, with_n=with_n, repeats=True)
    parts = [mutate_reads(rng, recs, 113 if e == 3 else 112 + (e == 0), m, e, sigma) for e in range(4)]
    parts.append(acgt(sigma)[rng.integers(0, 4, size=(50, m))])
    reads = np.concatenate(parts)
    assert len(reads) == 500
    reads = np.ascontiguousarray(reads[rng.permutation(len(reads))])
    pats = sa.interleave_rc(reads, sigma)
    schemes = [sa.search_scheme(gen, j, j, m) for j in range(k + 1)]
    ref = O.Index.build(recs, sigma, 16)
    want = hits_as_rows(O.search_best(ref, pats, schemes, nthreads=8))
    return dict(sigma=sigma, recs=recs, reads=reads, pats=pats, schemes=schemes, ref=ref, want=want)


_GPU = {}


def _gpu(case, device):
    """One resident index per text (keyed by the case's record list)."""
    key = (id(case["recs"]), device)
    if key not in _GPU:
        _GPU[key] = sa.BiFMIndex.build(case["recs"], sigma=case["sigma"], device=device)
    return _GPU[key]


def _all_calls(gpu, c, **kw):
    pk = sa.pack_reads(c["reads"], c["sigma"])
    yield "search_best", sa.search_best(gpu, c["pats"], c["schemes"])
    yield "search_best_reads", sa.search_best_reads(gpu, c["reads"], c["schemes"], **kw)
    yield "search_best_packed", sa.search_best_packed(gpu, pk, c["schemes"], **kw)
    yield "search_best_packed_compact", sa.search_best_packed_compact(gpu, pk, c["schemes"], **kw).to_hits()


@pytest.mark.parametrize("batch", ["7", "257", None])
@pytest.mark.parametrize("sigma", [6, 5])
def test_rounds_equal_oracle_over_batches(gpu_device, monkeypatch, sigma, batch):
    """Every entry point over 143 batches (cycling the 5 slots), 4 and 1, and
    the host loop (SAHARA_BEST_HOST=1) beside them."""
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = _case(sigma=sigma)
    gpu = _gpu(c, gpu_device)
    assert len(c["want"]) > len(c["pats"]) // 2
    for name, h in _all_calls(gpu, c):
        assert np.array_equal(hits_as_rows(h), c["want"]), name
        assert gpu.stats()["best_rounds"] == 3, name
    monkeypatch.setenv("SAHARA_BEST_HOST", "1")
    assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], c["schemes"])), c["want"])
    assert gpu.stats()["best_rounds"] == 0


def test_text_with_n_and_unequal_rounds(gpu_device, monkeypatch):
    """dna5 text with N runs; pigeon j = 0..3 at length 60: another number of
    searches in every round, and a text window planned for 3 errors used by
    the rounds with fewer."""
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = _case(with_n=True)
    for name, h in _all_calls(_gpu(c, gpu_device), c):
        assert np.array_equal(hits_as_rows(h), c["want"]), name
    c = _case(gen="pigeon", k=3, m=60, seed=6)
    assert len({len(s[0]) for s in c["schemes"]}) > 1
    gpu = _gpu(c, gpu_device)
    for name, h in _all_calls(gpu, c):
        assert np.array_equal(hits_as_rows(h), c["want"]), name
        assert gpu.stats()["best_rounds"] == 4, name


def test_no_reverse_and_odd_limit(gpu_device, monkeypatch):
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = _case()
    gpu = _gpu(c, gpu_device)
    fwd = hits_as_rows(O.search_best(c["ref"], c["reads"], c["schemes"], nthreads=8))
    for name, h in list(_all_calls(gpu, c, reverse=False))[1:]:
        assert np.array_equal(hits_as_rows(h), fwd), name
    # limit odd: the last read contributes only its forward strand
    cut = hits_as_rows(O.search_best(c["ref"], c["pats"][:333], c["schemes"], nthreads=8))
    for name, h in list(_all_calls(gpu, c, limit=333))[1:]:
        assert np.array_equal(hits_as_rows(h), cut), name


@pytest.mark.parametrize("batch", ["7", "257"])
@pytest.mark.parametrize("n", [1, 3])
def test_max_hits(gpu_device, monkeypatch, n, batch):
    from test_golden import limit_rows
    monkeypatch.setenv("SAHARA_BATCH", batch)
    c = _case()
    gpu = _gpu(c, gpu_device)
    want = limit_rows(c["want"], n)
    pk = sa.pack_reads(c["reads"], 6)
    assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], c["schemes"], max_hits=n)), want)
    assert np.array_equal(hits_as_rows(sa.search_best_reads(gpu, c["reads"], c["schemes"], max_hits=n)), want)
    assert np.array_equal(hits_as_rows(sa.search_best_packed(gpu, pk, c["schemes"], max_hits=n)), want)


@pytest.mark.parametrize("mode", ["fm_only", "lf_locate", "serial"])
def test_modes(gpu_device, monkeypatch, mode):
    """No text phase (the FM kernel alone feeds the mask), LF-walk locate,
    and every batch on one stream."""
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = _case()
    gpu = _gpu(c, gpu_device)
    try:
        if mode == "fm_only":
            gpu.set_mode(verify=False, locate_sa=True)
        elif mode == "lf_locate":
            gpu.set_mode(verify=True, locate_sa=False)
        else:
            monkeypatch.setenv("SAHARA_PIPELINE", "0")
        for name, h in _all_calls(gpu, c):
            assert np.array_equal(hits_as_rows(h), c["want"]), name
            assert gpu.stats()["pipelined"] == (0 if mode == "serial" else 1)
    finally:
        gpu.set_mode(verify=True, locate_sa=True)


@pytest.mark.parametrize("cap", ["SAHARA_HITCAP", "SAHARA_TASKCAP"])
def test_forced_overflow_rerun(gpu_device, monkeypatch, cap):
    """A hit / task buffer of one entry overflows in round 0: the pass is
    redone serially with grown buffers, every batch from its first round."""
    monkeypatch.setenv("SAHARA_BATCH", "257")
    monkeypatch.setenv(cap, "1")
    c = _case()
    gpu = sa.BiFMIndex.build(c["recs"], sigma=6, device=gpu_device)  # a fresh context: its buffers start at the cap
    for name, h in _all_calls(gpu, c):
        assert np.array_equal(hits_as_rows(h), c["want"]), name
    gpu.close()


def test_packed_shard_inside_a_byte(gpu_device, monkeypatch):
    monkeypatch.setenv("SAHARA_BATCH", "257")
    c = _case()
    gpu = _gpu(c, gpu_device)
    pk = sa.pack_reads(c["reads"], 6)
    r0, r1 = 101, 380
    assert r0 * pk.length % 4 != 0
    want = c["want"][(c["want"][:, 0] >= 2 * r0) & (c["want"][:, 0] < 2 * r1)].copy()
    want[:, 0] -= 2 * r0
    assert len(want)
    sh = pk.shard(r0, r1)
    assert np.array_equal(hits_as_rows(sa.search_best_packed(gpu, sh, c["schemes"])), want)
    assert np.array_equal(hits_as_rows(sa.search_best_packed_compact(gpu, sh, c["schemes"]).to_hits()), want)


@pytest.mark.parametrize("batch", ["257", None])
def test_mask_drops_items_on_the_device(gpu_device, monkeypatch, batch):
    """Count mode over the patterns a besthits call left staged: the seed
    kernel drops, in round j, every work item of a query that had a row after
    round j - 1. Filtering the hits afterwards would leave this at zero."""
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = _case()
    gpu = _gpu(c, gpu_device)
    found = np.zeros(len(c["pats"]), bool)
    want_skipped = 0
    for j, sch in enumerate(c["schemes"]):
        if j:
            want_skipped += int(found.sum()) * len(sch[0])
        h, _ = c["ref"].search(c["pats"], sch, edit=True, nthreads=8)
        found[np.unique(h[:, 0]).astype(np.int64)] = True
    assert 0 < found.sum() < len(found)
    sa.search_best_reads(gpu, c["reads"], c["schemes"])
    assert gpu.run(count=True) == len(c["want"])
    st = gpu.stats()
    assert st["best_rounds"] == 3
    assert st["best_skipped"] == want_skipped
    assert np.array_equal(hits_as_rows(gpu.fetch()), c["want"])
    # an all-mode pass has one round and no mask
    sa.search_reads(gpu, c["reads"], sa.search_scheme("h2-k2", 0, 2, 50))
    gpu.run(count=True)
    assert gpu.stats()["best_rounds"] == 0 and gpu.stats()["best_skipped"] == 0


def test_multi_part_index_takes_the_host_loop(gpu_device, monkeypatch):
    """"Found" is decided across the parts: the whole-hit calls interleave into
    ranks and run the host loop there (correct results, no rounds), the
    compact call refuses as its all-mode twin does."""
    c = _case(with_n=True)
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "9000")
    gpu = sa.BiFMIndex.build(c["recs"], sigma=6, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    assert gpu.info()["n_parts"] > 1
    pk = sa.pack_reads(c["reads"], 6)
    cut = hits_as_rows(O.search_best(c["ref"], c["pats"][:333], c["schemes"], nthreads=8))
    for name, fn, arg in (("reads", sa.search_best_reads, c["reads"]), ("packed", sa.search_best_packed, pk)):
        assert np.array_equal(hits_as_rows(fn(gpu, arg, c["schemes"])), c["want"]), name
        assert gpu.stats()["best_rounds"] == 0, name
        assert np.array_equal(hits_as_rows(fn(gpu, arg, c["schemes"], limit=333)), cut), name
    assert np.array_equal(hits_as_rows(sa.search_best(gpu, c["pats"], c["schemes"])), c["want"])
    with pytest.raises(sa.SaharaError, match="single-part index"):
        sa.search_best_packed_compact(gpu, pk, c["schemes"])
    gpu.close()


def test_guard_rails(gpu_device):
    c = _case()
    gpu = _gpu(c, gpu_device)
    pk = sa.pack_reads(c["reads"], 6)
    calls = [lambda s: sa.search_best(gpu, c["pats"], s),
             lambda s: sa.search_best_reads(gpu, c["reads"], s),
             lambda s: sa.search_best_packed(gpu, pk, s),
             lambda s: sa.search_best_packed_compact(gpu, pk, s)]
    for call in calls:
        with pytest.raises(sa.SaharaError, match="no schemes"):
            call([])
    # 17 schemes: j = 16 is more than compact records (and the kernels) hold
    pi, l, u = c["schemes"][2]
    many = [(pi, np.minimum(l, j), np.where(u > 0, j, 0).astype(np.uint32)) for j in range(17)]
    with pytest.raises(sa.SaharaError, match="15 errors"):
        sa.search_best_packed_compact(gpu, pk, many)
    # a pattern length shorter than the scheme's parts
    with pytest.raises(sa.SaharaError, match="cannot expand"):  # (the wrappers' schemes never get that far)
        sa.search_scheme("h2-k2", 2, 2, 2)
    short = sa.PackedReads(pk.codes, 100, 2)
    wide = [(np.zeros((1, 3), np.uint32), np.zeros((1, 3), np.uint32), np.zeros((1, 3), np.uint32))]
    for call in (lambda: sa.search_best_packed(gpu, short, wide),
                 lambda: sa.search_best_packed_compact(gpu, short, wide),
                 lambda: sa.search_best_reads(gpu, c["reads"][:, :2], wide)):
        with pytest.raises(sa.SaharaError):
            call()
    # the context still works
    assert np.array_equal(hits_as_rows(sa.search_best_reads(gpu, c["reads"], c["schemes"])), c["want"])
