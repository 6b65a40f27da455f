"""Streamed calls whose sink takes compact records sort each batch straight
into them (locate_sort.hip kSortDecode<true>, kSortBigLds<true>, kDecodeBig<true>;
pass.cpp finish): no whole hit of such a batch is written on the device until
a reader of the whole hits asks (Ctx::wholeHits: fetch, digest). Every sort
tier over several batches, a sink that is too small and refilled from the
device-resident records, the Expander route, the lazy decode, the routes that
keep the whole-record sort (--max_hits, multi-part indexes), and texts of one
and of more than 256 records. The oracle is the reference throughout; records
are compared row for row, in order."""
import functools

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows, mutate_reads, random_records

pytestmark = pytest.mark.gpu


def _ordered(h):
    return np.stack([h["qid"], h["seq_id"], h["pos"], h["err"]], 1).astype(np.uint64)


def _compact(call, *args, **kw):
    c = call(*args, **kw)
    rows = _ordered(c.to_hits())
    c.close()
    return rows


# units tiled this often: exact patterns of a unit have about as many rows
# (a few more with one error), which puts segments on both sides of the sort's
# tier boundaries 8 | 9, 64 | 65 and 2048 | 2049
TILES = (3, 7, 8, 9, 12, 40, 62, 64, 65, 70, 700, 1500, 2040, 2060, 2600)


@functools.lru_cache(maxsize=None)
def _tier_case():
    """test_long_and_huge_segments' shape with more tile counts: a
    repeat-rich text and patterns (qid = row) whose segments take every tier
    of the sort, with the oracle's rows."""
    rng = np.random.default_rng(177)
    recs, pats = [], []
    for tiles in TILES:
        unit = random_records(rng, [50], 6)[0]
        r = np.tile(unit, tiles)
        if tiles > 100:
            r[rng.integers(0, len(r), tiles // 100)] = rng.integers(1, 6, tiles // 100)
        recs.append(r)
        for s in rng.integers(0, 50, 6):
            p = np.roll(unit, -int(s))[:24].copy()
            if s % 2:
                p[rng.integers(0, 24)] = rng.integers(1, 6)
            pats.append(p)
    pats = np.vstack(pats + random_records(rng, [24] * 8, 6)).astype(np.uint8)
    pats = pats[rng.permutation(len(pats))]
    sch = sa.search_scheme("h2-k1", 0, 1, 24)
    want = hits_as_rows(O.Index.build(recs, 6, 16).search(pats, sch, nthreads=8)[0])
    want.setflags(write=False)
    return recs, pats, sch, want


def test_tier_case_covers_every_boundary(gpu_device):
    """(no GPU work) the shared case has segments in every tier and close to
    both sides of every boundary between two tiers"""
    _, pats, _, want = _tier_case()
    per_q = np.bincount(want[:, 0].astype(np.int64), minlength=len(pats))
    for lo, hi in ((1, 8), (9, 16), (33, 64), (65, 128), (1025, 2048), (2049, 4096), (4097, 1 << 30)):
        assert ((per_q >= lo) & (per_q <= hi)).any(), (lo, hi)
    assert (per_q == 0).any()


@pytest.mark.parametrize("batch", ["29", "1000000"])
def test_every_sort_tier_over_batches(gpu_device, monkeypatch, batch):
    """Compact records of the reads and the packed call, expanded, equal the
    oracle's hits row for row and the whole-record call's, in four batches (of
    29 patterns) and in one."""
    monkeypatch.setenv("SAHARA_BATCH", batch)
    recs, pats, sch, want = _tier_case()
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    whole = _ordered(sa.search_reads(gpu, pats, sch, reverse=False))
    assert np.array_equal(whole, want)
    for _ in range(2):  # the sink from the estimate, then sized from the last call
        c = sa.search_reads_compact(gpu, pats, sch, reverse=False)
        assert len(c.block_end) == (4 if batch == "29" else 1)
        assert np.array_equal(_ordered(c.to_hits()), want)
        c.close()
    packed = sa.pack_reads(pats, 6, pinned=True)
    assert np.array_equal(_compact(sa.search_packed_compact, gpu, packed, sch, reverse=False), want)
    # with reverse complements (two patterns per read) the same holds
    want_rc = hits_as_rows(sa.search_reads(gpu, pats[:40], sch))
    assert np.array_equal(_compact(sa.search_reads_compact, gpu, pats[:40], sch), want_rc)


@pytest.mark.parametrize("pin_min", [None, "0"])
def test_first_call_sink_too_small_is_refilled(gpu_device, monkeypatch, pin_min):
    """A fresh context's first compact call sizes its sink for two hits per
    pattern; with thousands of rows per pattern it overflows mid-pass, and the
    call's records come again from the device-resident compact records: the
    same records as the second call's (whose sink fits), and the oracle's.
    SAHARA_PIN_MIN (the knob of test_pinned_hit_sink_grows_and_is_recycled)
    set and unset; the compact call's sink is page-locked whatever its size,
    so the copy-out into a pageable sink is reached only when page-locking
    fails, which no knob forces. Three held results first take every idle
    buffer out of the library's pool, so that the sink is a new one of the
    estimate's size (2 MiB: 262144 records)."""
    if pin_min is not None:
        monkeypatch.setenv("SAHARA_PIN_MIN", pin_min)
    monkeypatch.setenv("SAHARA_BATCH", "16")
    recs, pats, sch, want = _tier_case()
    per_q = np.bincount(want[:, 0].astype(np.int64), minlength=len(pats))
    reads = np.repeat(pats[per_q > 2048], 5, axis=0)  # 5 copies of every huge-segment pattern
    ref = O.Index.build(recs, 6, 16)
    want = hits_as_rows(ref.search(reads, sch, nthreads=8)[0])
    assert len(want) > 262144 + 16 * per_q.max()  # past the sink while batches are still to come
    tiny = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    held = [sa.search_reads_compact(tiny, pats[:4], sch, reverse=False) for _ in range(3)]
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    first = sa.search_reads_compact(gpu, reads, sch, reverse=False)
    assert len(first.block_end) > 3
    second = sa.search_reads_compact(gpu, reads, sch, reverse=False)
    assert np.array_equal(first.recs, second.recs)
    assert np.array_equal(first.block_end, second.block_end)
    assert np.array_equal(_ordered(first.to_hits()), want)
    for c in held + [first, second]:
        c.close()


def test_expander_route_equals_oracle(gpu_device, monkeypatch):
    """sahara_gpu_search with a pageable sink and the compact download (host
    threads expand each batch's records): the oracle's hits, and the
    device-resident hits afterwards (fetch) too."""
    monkeypatch.setenv("SAHARA_COMPACT_DOWNLOAD", "1")
    monkeypatch.setenv("SAHARA_BATCH", "29")
    recs, pats, sch, want = _tier_case()
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    for _ in range(2):
        assert np.array_equal(_ordered(sa.search(gpu, pats, sch)), want)
    assert np.array_equal(_ordered(gpu.fetch()), want)
    assert np.array_equal(_ordered(sa.search_reads(gpu, pats, sch, reverse=False)), want)


def test_lazy_decode_after_a_compact_call(gpu_device, monkeypatch):
    """fetch() and digest() straight after a compact call equal those after
    the whole-record call on the same input, whichever comes first, and a
    second fetch gives the same."""
    monkeypatch.setenv("SAHARA_BATCH", "29")
    recs, pats, sch, want = _tier_case()
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    monkeypatch.setenv("SAHARA_FULL_DOWNLOAD", "1")
    sa.search_reads(gpu, pats, sch, reverse=False)
    whole_digest, whole = gpu.digest(), gpu.fetch()
    monkeypatch.delenv("SAHARA_FULL_DOWNLOAD")
    assert np.array_equal(_ordered(whole), want)
    sa.search_reads_compact(gpu, pats, sch, reverse=False).close()
    assert gpu.digest() == whole_digest
    assert np.array_equal(gpu.fetch(), whole)
    sa.search_packed_compact(gpu, sa.pack_reads(pats, 6), sch, reverse=False).close()
    assert np.array_equal(gpu.fetch(), whole)
    assert np.array_equal(gpu.fetch(), whole)
    assert gpu.digest() == whole_digest
    # the staged patterns run again device-resident: whole records once more
    gpu.run()
    assert np.array_equal(gpu.fetch(), whole)


def test_max_hits_keeps_the_whole_record_route(gpu_device, monkeypatch):
    """--max_hits limits whole hits on the device, so its batches are not
    sorted into compact records although the sink takes them (the compact
    download): the documented policy over the oracle's hits. (The compact
    entry points themselves take no max_hits.)"""
    from test_golden import limit_rows
    monkeypatch.setenv("SAHARA_COMPACT_DOWNLOAD", "1")
    monkeypatch.setenv("SAHARA_BATCH", "29")
    recs, pats, sch, want = _tier_case()
    sel = np.flatnonzero(np.bincount(want[:, 0].astype(np.int64), minlength=len(pats)) <= 200)
    want3 = limit_rows(hits_as_rows(O.Index.build(recs, 6, 16).search(pats[sel], sch, nthreads=8)[0]), 3)
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    assert np.array_equal(_ordered(sa.search(gpu, pats, sch)), want)  # a compact-record call first
    assert np.array_equal(hits_as_rows(sa.search(gpu, pats[sel], sch, max_hits=3)), want3)
    assert np.array_equal(hits_as_rows(sa.search_reads(gpu, pats[sel], sch, reverse=False, max_hits=3)), want3)
    assert np.array_equal(hits_as_rows(gpu.fetch()), want3)


def test_multi_part_index_keeps_the_whole_record_route(gpu_device, monkeypatch):
    """An index in parts merges whole hits after its parts' passes: the
    compact download gives the oracle's hits, and the compact entry points
    refuse it as before."""
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "200000")
    monkeypatch.setenv("SAHARA_COMPACT_DOWNLOAD", "1")
    monkeypatch.setenv("SAHARA_BATCH", "29")
    recs, pats, sch, want = _tier_case()
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    assert gpu.info()["n_parts"] > 1
    assert np.array_equal(hits_as_rows(sa.search(gpu, pats, sch)), want)
    assert np.array_equal(hits_as_rows(gpu.fetch()), want)
    with pytest.raises(sa.SaharaError, match="single-part"):
        sa.search_reads_compact(gpu, pats, sch, reverse=False)
    with pytest.raises(sa.SaharaError, match="single-part"):
        sa.search_packed_compact(gpu, sa.pack_reads(pats, 6), sch, reverse=False)
    assert np.array_equal(hits_as_rows(sa.search_reads(gpu, pats, sch, reverse=False)), want)


@pytest.mark.parametrize("nrec", [1, 256, 257, 700])
def test_texts_of_one_and_of_many_records(gpu_device, monkeypatch, nrec):
    """The compact form reads no record starts; the lazy decode does, from
    LDS (<= 256 records) and from global memory (more)."""
    monkeypatch.setenv("SAHARA_BATCH", "700")
    rng = np.random.default_rng(nrec)
    recs = random_records(rng, [40000] if nrec == 1 else list(rng.integers(30, 160, size=nrec)), 6)
    m, k = 30, 2
    reads = mutate_reads(rng, recs, 1000, m, k)
    sch = sa.search_scheme("h2-k2", 0, k, m)
    want = hits_as_rows(O.Index.build(recs, 6, 16).search(sa.interleave_rc(reads, 6), sch, nthreads=8)[0])
    assert len(np.unique(want[:, 1])) > nrec // 2
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    assert gpu.info()["n_records"] == nrec
    c = sa.search_reads_compact(gpu, reads, sch)
    assert len(c.block_end) == 3
    assert np.array_equal(_ordered(c.to_hits()), want)
    c.close()
    assert np.array_equal(_ordered(gpu.fetch()), want)
    assert np.array_equal(_compact(sa.search_packed_compact, gpu, sa.pack_reads(reads, 6), sch), want)
    assert np.array_equal(_ordered(gpu.fetch()), want)
