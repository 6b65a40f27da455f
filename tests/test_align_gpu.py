"""kAlignHits on the device against tests/align_model.py: every record equal
field by field, every record replayed (apply). Hits come from the search
calls themselves (duplicates included), from reads sampled where the window
meets a '$', the pad after the text or every shift of a text block, and from
positions the caller made up (the only way to a NONE record)."""
import ctypes as C

import numpy as np
import pytest

import align_model as am
import sahara_amd as sa
from helpers import hits_as_rows, mutate_reads, pset, random_records

pytestmark = pytest.mark.gpu

SHORT = 15  # a record shorter than every m below


def make_records(sigma):
    rng = np.random.default_rng(40 + sigma)
    recs = random_records(rng, [3000, SHORT, 1200, 700], sigma, with_n=True)
    a = recs[0]
    a[400:560] = a[400]                                  # a homopolymer stretch
    a[900:1080] = np.resize(a[897:900], 180)             # a period-3 stretch: ties in the traceback
    if sigma == 6:
        a[1500:1507] = 4                                 # N runs
        recs[2][300:303] = 4
    return recs


_CACHE = {}


def world(sigma, device):
    """(records, text, record starts, index) per alphabet, built once."""
    if sigma not in _CACHE:
        recs = make_records(sigma)
        T = am.concat_text(recs)
        starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])]).astype(np.int64)
        _CACHE[sigma] = (recs, T, starts, sa.BiFMIndex.build(recs, sigma=sigma, device=device))
    return _CACHE[sigma]


_MODEL = {}


def model(P, T, g, K, edit, key):
    k = (key, P.tobytes(), g, K, edit)
    if k not in _MODEL:
        res = am.align(P.tolist(), T, g, K, edit)
        if res is not None:
            assert am.apply(P.tolist(), T, g, res[1], res[2])
        _MODEL[k] = am.record_of(res)
    return _MODEL[k]


def check_records(got, pats, hits, T, starts, K, edit, key, allow_none=False):
    assert len(got) == len(hits)
    n_none = 0
    for r, h in zip(got, hits):
        g = int(starts[int(h["seq_id"])]) + int(h["pos"])
        e, ref_len, words = model(pats[int(h["qid"])], T, g, K, edit, key)
        assert (int(r["err"]), int(r["ref_len"]), r["edit"].tolist()) == (e, ref_len, words), (h, r)
        n_none += e == am.NONE
    assert allow_none or n_none == 0
    return n_none


def thin(hits, cap):
    return hits if len(hits) <= cap else hits[:: -(-len(hits) // cap)]


@pytest.mark.parametrize("m", [20, 32, 33, 64, 100, 250])
@pytest.mark.parametrize("K", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("edit", [True, False])
def test_hits_of_the_search_align_as_the_model(gpu_device, m, K, edit):
    sigma = 6 if (m + K) % 2 == 0 else 5
    recs, T, starts, gpu = world(sigma, gpu_device)
    rng = np.random.default_rng(1000 * m + 10 * K + edit)
    # reads out of the homopolymer and period-3 stretches of record 0 only up to K = 2: in all-mode the
    # search itself enumerates every placement of the edits inside such a stretch, which at K = 4 and
    # m = 250 takes it minutes (the stretches stay in the text, and the made-up hits below land in them)
    sources = [recs[0], recs[2], recs[3]] if K <= 2 else [recs[2], recs[3]]
    if edit:
        reads = mutate_reads(rng, sources, 120, m, K, sigma)
    else:  # -d ham finds no read with an indel: up to K substitutions instead
        reads = mutate_reads(rng, sources, 120, m, 0, sigma)
        for r in reads:
            for j in rng.integers(0, m, size=K):
                r[j] = rng.choice([1, 2, 3])
    pats = sa.interleave_rc(reads, sigma)
    sch = sa.search_scheme("pigeon", 0, K, m, hamming=not edit)
    hits = sa.search(gpu, pats, sch, edit=edit)
    assert len(hits) >= len(reads) // 2
    best = pset(hits_as_rows(hits))
    hits = thin(hits, 700 if m > 100 else 2500)
    got = sa.align(gpu, pats, hits, edit=edit, max_err=K)
    check_records(got, pats, hits, T, starts, K, edit, sigma)
    for r, h in zip(got, hits):  # e* is the P-set's e of the position
        assert int(r["err"]) == best[(int(h["qid"]), int(h["seq_id"]), int(h["pos"]))]
    if not edit:
        assert (got["ref_len"] == m).all() and ((got["edit"] & 3) <= 1).all()


@pytest.mark.parametrize("m,K", [(33, 2), (100, 3)])
def test_positions_at_block_shifts_record_ends_text_end_and_start(gpu_device, m, K):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(m)
    places = [(0, 0)]                                                     # pos 0 of record 0
    places += [(0, 2000 + i) for i in range(32)]                          # every shift of a text block
    places += [(s, len(recs[s]) - m - d) for s in (0, 2) for d in range(0, K + 2)]  # the window meets '$'
    places += [(3, len(recs[3]) - m - d) for d in range(0, K + 2)]        # ... and the pad after the text
    reads = np.stack([recs[s][p:p + m] for s, p in places]).copy()
    for i in range(len(reads)):                                           # true reads, most with an edit
        if i % 3:
            j = int(rng.integers(1, m - 1))
            reads[i, j] = 1 + reads[i, j] % 3
    sch = sa.search_scheme("pigeon", 0, K, m)
    hits = sa.search(gpu, reads, sch, edit=True)
    at = {(int(h["qid"]), int(h["seq_id"]), int(h["pos"])) for h in hits}
    for q, (s, p) in enumerate(places):
        assert (q, s, p) in at
    g = starts[hits["seq_id"].astype(np.int64)] + hits["pos"].astype(np.int64)
    assert set((g % 32).tolist()) == set(range(32))
    assert (g + m + K > len(T) - 1).any() and (g == 0).any()
    got = sa.align(gpu, reads, hits, edit=True, max_err=K)
    check_records(got, reads, hits, T, starts, K, True, 6)


def test_max_err_at_its_largest(gpu_device):
    recs, T, starts, gpu = world(5, gpu_device)
    rng = np.random.default_rng(8)
    m = 40
    reads = mutate_reads(rng, [recs[0], recs[2]], 30, m, 4, 5)
    sch = sa.search_scheme("backtracking", 0, 4, m)
    hits = thin(sa.search(gpu, reads, sch, edit=True), 2500)
    assert len(hits) > 30
    got = sa.align(gpu, reads, hits, edit=True, max_err=sa.ALIGN_MAX_ERR)
    check_records(got, reads, hits, T, starts, sa.ALIGN_MAX_ERR, True, 5)


def made_up_hits(rng, recs, n_pats, n):
    hits = np.zeros(n, sa.HIT_DTYPE)
    hits["qid"] = rng.integers(0, n_pats, size=n)
    hits["seq_id"] = rng.integers(0, len(recs), size=n)
    hits["pos"] = [rng.integers(0, len(recs[s])) for s in hits["seq_id"]]
    hits["err"] = rng.integers(0, 9, size=n)  # (ignored by the call)
    return hits


def test_hits_the_caller_made_up(gpu_device):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(77)
    m, K = 50, 3
    reads = mutate_reads(rng, [recs[0], recs[2], recs[3]], 60, m, 2, 6)
    sch = sa.search_scheme("h2-k2", 0, 2, m)
    true = sa.search(gpu, reads, sch, edit=True)
    near = true[rng.integers(0, len(true), size=800)].copy()  # around true positions: some align, some do not
    shift = rng.integers(-4, 5, size=len(near))
    lens = np.array([len(r) for r in recs])[near["seq_id"]]
    near["pos"] = np.clip(near["pos"].astype(np.int64) + shift, 0, lens - 1)
    hits = np.concatenate([near, made_up_hits(rng, recs, len(reads), 1200)])
    hits = hits[rng.permutation(len(hits))]                   # any order
    got = sa.align(gpu, reads, hits, edit=True, max_err=K)
    n_none = check_records(got, reads, hits, T, starts, K, True, 6, allow_none=True)
    assert 100 < n_none < len(hits) - 100
    none = got[got["err"] == sa.ALIGN_NONE]
    assert (none["ref_len"] == 0).all() and (none["edit"] == 0).all()


def test_hits_out_of_range_are_refused_and_out_is_untouched(gpu_device):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(3)
    m = 30
    reads = mutate_reads(rng, [recs[0]], 8, m, 1, 6)
    good = made_up_hits(rng, recs, len(reads), 50)
    L = sa.lib()

    def call(hits, n_pats=len(reads), length=m, max_err=2):
        out = np.full(len(hits), 0x5A, np.uint8).repeat(24).view(sa.ALIGN_DTYPE)
        keep = out.copy()
        q = np.ascontiguousarray(reads)
        rc = L.sahara_gpu_align(gpu._h, q.ctypes.data_as(sa.u8p), n_pats, length, 1, max_err,
                                hits.ctypes.data_as(C.c_void_p), len(hits), out.ctypes.data_as(C.c_void_p))
        return rc, L.sahara_gpu_last_error().decode(), np.array_equal(out.view(np.uint8), keep.view(np.uint8))

    rc, _, same = call(good)
    assert rc == 0 and not same
    for field, value, what in (("qid", len(reads), "pattern"), ("qid", 2 ** 40, "pattern"),
                               ("seq_id", len(recs), "record"), ("seq_id", 2 ** 32 - 1, "record")):
        bad = good.copy()
        bad[field][37] = value
        rc, msg, same = call(bad)
        assert rc < 0 and what in msg and "hit 37" in msg and same, (field, value, msg)
    bad = good.copy()
    bad["seq_id"][49], bad["pos"][49] = 1, SHORT  # one past the record's last symbol (its '$')
    rc, msg, same = call(bad)
    assert rc < 0 and "position" in msg and "hit 49" in msg and same
    bad["pos"][49] = 2 ** 63
    rc, msg, same = call(bad)
    assert rc < 0 and same
    rc, msg, same = call(good, max_err=sa.ALIGN_MAX_ERR + 1)
    assert rc < 0 and "max_err" in msg and same
    for length in (0, 16384):
        rc, msg, same = call(good, length=length)
        assert rc < 0 and "length" in msg and same


def test_chunks_of_any_size_give_the_same_records(gpu_device, monkeypatch):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(21)
    m, K = 64, 2
    reads = mutate_reads(rng, [recs[0], recs[2], recs[3]], 50, m, K, 6)
    hits = made_up_hits(rng, recs, len(reads), 2000)
    hits = np.concatenate([sa.search(gpu, reads, sa.search_scheme("h2-k2", 0, K, m)), hits])[:5000]
    monkeypatch.delenv("SAHARA_ALIGN_CHUNK", raising=False)
    whole = sa.align(gpu, reads, hits, max_err=K)
    assert sa.align_stats(gpu)["chunks"] == 1 and sa.align_stats(gpu)["hits"] == len(hits)
    check_records(whole, reads, hits, T, starts, K, True, 6, allow_none=True)
    for chunk in (1, 1000):
        monkeypatch.setenv("SAHARA_ALIGN_CHUNK", str(chunk))
        got = sa.align(gpu, reads, hits, max_err=K)
        assert sa.align_stats(gpu)["chunks"] == -(-len(hits) // chunk)
        assert np.array_equal(got.view(np.uint8), whole.view(np.uint8))


@pytest.mark.parametrize("reverse,limit,shard", [(True, 0, None), (False, 0, None), (True, 41, None),
                                                 (True, 0, (3, 29)), (False, 17, (5, 40))])
def test_packed_entry_equals_align_on_the_whole_hits(gpu_device, monkeypatch, reverse, limit, shard):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(12)
    m, K = 33, 2                                 # m odd: a shard starts inside a byte
    reads = mutate_reads(rng, [recs[0], recs[2], recs[3]], 48, m, K, 6)
    reads[::5] = recs[0][1490:1490 + m]          # reads with N
    reads[7] = recs[2][290:290 + m]
    packed = sa.pack_reads(reads, 6)
    assert packed.n_pos.size > 10
    if shard:
        packed = packed.shard(*shard)
        assert packed.sym0 % 4 != 0
        reads = reads[shard[0]:shard[1]]
    pats = sa.interleave_rc(reads, 6) if reverse else reads
    if limit:
        assert limit % 2 == 1 or not reverse  # cuts inside a read pair
        pats = pats[:limit]
    sch = sa.search_scheme("h2-k2", 0, K, m)
    monkeypatch.setenv("SAHARA_BATCH", "7")      # several blocks
    c = sa.search_packed_compact(gpu, packed, sch, edit=True, reverse=reverse, limit=limit)
    assert len(c) > len(pats) // 2 and len(c.block_end) > 1
    hits = c.to_hits()
    assert np.array_equal(hits_as_rows(hits), hits_as_rows(sa.search(gpu, pats, sch)))
    monkeypatch.setenv("SAHARA_ALIGN_CHUNK", "333")
    got = sa.align_packed_compact(gpu, packed, c, edit=True, reverse=reverse, limit=limit, max_err=K)
    want = sa.align(gpu, pats, hits, edit=True, max_err=K)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    check_records(got, pats, hits, T, starts, K, True, 6)
    c.close()


def test_packed_entry_refuses_records_beyond_the_call(gpu_device):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(13)
    m = 40
    reads = mutate_reads(rng, [recs[0]], 20, m, 1, 6)
    packed = sa.pack_reads(reads, 6)
    c = sa.search_packed_compact(gpu, packed, sa.search_scheme("h2-k1", 0, 1, m))
    with pytest.raises(sa.SaharaError, match="pattern"):
        sa.align_packed_compact(gpu, packed.shard(0, 5), c, max_err=1)  # fewer reads than the records name
    with pytest.raises(sa.SaharaError, match="max_err"):
        sa.align_packed_compact(gpu, packed, c, max_err=9)
    c.close()


def test_multi_part_index_aligns_as_one_part(gpu_device, monkeypatch):
    recs, T, starts, one = world(6, gpu_device)
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "1500")  # records 0 | 1, 2 | 3
    parts = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    monkeypatch.delenv("SAHARA_PART_SYMBOLS")
    assert parts.info()["n_parts"] == 3
    rng = np.random.default_rng(31)
    m, K = 70, 2
    reads = mutate_reads(rng, [recs[0], recs[2], recs[3]], 90, m, K, 6)
    sch = sa.search_scheme("h2-k2", 0, K, m)
    hits = sa.search(parts, reads, sch)
    assert np.array_equal(hits_as_rows(hits), hits_as_rows(sa.search(one, reads, sch)))
    assert set(hits["seq_id"].tolist()) == {0, 2, 3}
    hits = np.concatenate([hits, made_up_hits(rng, recs, len(reads), 300)])
    monkeypatch.setenv("SAHARA_ALIGN_CHUNK", "500")
    got = sa.align(parts, reads, hits, max_err=K)
    want = sa.align(one, reads, hits, max_err=K)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    check_records(got, reads, hits, T, starts, K, True, 6, allow_none=True)
    c = sa.search_packed_compact(one, sa.pack_reads(reads, 6), sch, reverse=False)
    with pytest.raises(sa.SaharaError, match="single-part index"):
        sa.align_packed_compact(parts, sa.pack_reads(reads, 6), c, reverse=False, max_err=K)
    c.close()


def test_besthits_and_max_hits_align_too(gpu_device):
    recs, T, starts, gpu = world(6, gpu_device)
    rng = np.random.default_rng(55)
    m, K = 60, 2
    reads = mutate_reads(rng, [recs[0], recs[2], recs[3]], 120, m, K, 6)
    pats = sa.interleave_rc(reads, 6)
    best = sa.search_best(gpu, pats, [sa.search_scheme("h2-k2", j, j, m) for j in range(K + 1)])
    few = sa.search(gpu, pats, sa.search_scheme("h2-k2", 0, K, m), max_hits=2)
    assert len(best) > 100 and len(few) > 100
    for hits in (best, few):
        hits = thin(hits, 2500)
        got = sa.align(gpu, pats, hits, max_err=K)
        check_records(got, pats, hits, T, starts, K, True, 6)
        assert (got["err"] <= hits["err"]).all()  # these calls report each position with its least e
