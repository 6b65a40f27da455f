"""The index kernels (index_build.hip) and kLocate's LF walk (locate_sort.hip) at
other sampling rates and at the sizes where they change path.

The case table is tests/index_cases.py's; what every case must give is the
from-scratch model of tests/index_model.py (a naive sort of the suffixes),
which tests/test_index_model.py holds the oracle to without a GPU. Here:

- build parity: sahara_gpu_build's SA, text, BWTs, sampled bits, samples, C and
  record lengths equal the model's, at rates 1 .. 1000 (kSampledBits, kSamples),
  at N on and next to the edges of kPackText (32), the Occ lines (64, and the
  extra empty line when 64 | N), kLinesLocal's fast path and kDensify's
  geometry (16, 1024, 4096), and with LCPs on the prefix-doubling steps;
- load parity: the oracle's .idx at that rate, densified on load (kDensify's
  walk bound is the rate), exports the model's SA and text; the saved GPU
  build is the oracle's file byte for byte;
- locate: hits and the counted LF steps equal the oracle's on built and loaded
  contexts (kLocate's bound and sample index; lf_steps is 0 at rate 1 and
  grows with the rate, so neither can hide);
- degenerate texts searched: records around the pattern length, empty records,
  the N = 2 index, patterns longer than every record;
- an .idx whose rate field is 0 or does not fit 32 bits is refused.

Every text has at most 8193 symbols, every search at most 100 patterns.
"""
import contextlib
import functools
import os
import tempfile

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows, mutate_reads, pset
from index_cases import (BY_ID, CASES, DEGENERATE, LOCATE_CASES, LOCATE_K, LOCATE_M, TINY, degenerate, locate_inputs,
                         oracle_index, rate_offset, records, reference, tiny)

pytestmark = pytest.mark.gpu

MODES = [(True, True), (False, False), (True, False), (False, True)]  # (verify, locate_sa)


@functools.lru_cache(maxsize=None)
def oracle_image(case_id):
    """The oracle-written .idx of a case, as bytes."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "oracle.idx")
        oracle_index(case_id).write(path)
        with open(path, "rb") as f:
            return f.read()


def built(case_id, device):
    c = BY_ID[case_id]
    return contextlib.closing(sa.BiFMIndex.build(list(records(case_id)), sigma=c.sigma, sampling_rate=c.rate,
                                                 device=device))


def loaded(case_id, device):
    return contextlib.closing(sa.BiFMIndex.from_bytes(oracle_image(case_id), device=device))


def assert_is_model(gpu, case_id):
    c, want = BY_ID[case_id], reference(case_id)
    inf = gpu.info()
    assert (inf["n"], inf["n_records"], inf["n_samples"], inf["sampling_rate"], inf["sigma"], inf["n_parts"]) == \
        (want["n"], want["n_records"], want["n_samples"], c.rate, c.sigma, 1)
    assert np.array_equal(gpu.export_sa(), want["sa"])
    assert np.array_equal(gpu.export_text(), want["text"])
    got = gpu.export()
    for key in ("bwt_f", "bwt_r", "sampled", "samples", "C", "rec_lens"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["rate"] == c.rate


@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_build_equals_model(gpu_device, case_id):
    with built(case_id, gpu_device) as gpu:
        assert_is_model(gpu, case_id)


@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_load_equals_model_and_save_equals_oracle_file(gpu_device, tmp_path, case_id):
    """from_bytes of the oracle's file rebuilds the full SA and the text from
    the samples (kDensify) at the file's rate; the GPU build saves that file."""
    image = oracle_image(case_id)
    at = rate_offset(BY_ID[case_id].sigma, len(records(case_id)))
    assert int.from_bytes(image[at:at + 8], "little") == BY_ID[case_id].rate
    with loaded(case_id, gpu_device) as gpu:
        assert_is_model(gpu, case_id)
    with built(case_id, gpu_device) as gpu:
        gpu.save(tmp_path / "gpu.idx")
    assert (tmp_path / "gpu.idx").read_bytes() == image


def assert_locates_like_oracle(gpu, case_id, label):
    pats, want, cnt = locate_inputs(case_id)
    sch = sa.search_scheme("h2-k2", 0, LOCATE_K, LOCATE_M)
    for verify, locate_sa in MODES:
        gpu.set_mode(verify=verify, locate_sa=locate_sa)
        assert np.array_equal(hits_as_rows(sa.search(gpu, pats, sch)), want), (verify, locate_sa)
    gpu.set_mode(verify=False, locate_sa=False)  # every node ranked, every row located by an LF walk
    gpu.stage(pats, sch, edit=True)
    assert gpu.run(count=True) == len(want)
    st = gpu.stats()
    print(f"lf_steps {case_id} {label}: gpu {st['lf_steps']} oracle {cnt['lf_steps']}")
    assert (st["lf_steps"], st["nodes"], st["cursors"]) == (cnt["lf_steps"], cnt["nodes"], cnt["leaves"])
    assert np.array_equal(hits_as_rows(gpu.fetch()), want)


@pytest.mark.parametrize("case_id", [c.id for c in LOCATE_CASES])
def test_locate_on_built_index(gpu_device, case_id):
    with built(case_id, gpu_device) as gpu:
        assert_locates_like_oracle(gpu, case_id, "built")


@pytest.mark.parametrize("case_id", [c.id for c in LOCATE_CASES])
def test_locate_on_loaded_index(gpu_device, case_id):
    with loaded(case_id, gpu_device) as gpu:
        assert_locates_like_oracle(gpu, case_id, "loaded")


def test_locate_multi_part_at_rate_5(gpu_device, monkeypatch, tmp_path):
    """Three parts (SAHARA_PART_SYMBOLS) at rate 5, built and loaded from their
    saved file: the hits of the single-part index of the same text, which are
    the oracle's."""
    recs = list(records("rate16-s6"))
    rng = np.random.default_rng(55)
    pats = mutate_reads(rng, recs, 100, 24, 2, 6)
    sch = sa.search_scheme("h2-k2", 0, 2, 24)
    want = hits_as_rows(O.Index.build(recs, 6, 5).search(pats, sch)[0])
    monkeypatch.setenv("SAHARA_PART_SYMBOLS", "1200")
    with contextlib.closing(sa.BiFMIndex.build(recs, sigma=6, sampling_rate=5, device=gpu_device)) as parts:
        monkeypatch.delenv("SAHARA_PART_SYMBOLS")
        inf = parts.info()
        assert (inf["n_parts"], inf["sampling_rate"], inf["n"]) == (3, 5, reference("rate16-s6")["n"])
        parts.save(tmp_path / "parts.idx")
        with contextlib.closing(sa.BiFMIndex.build(recs, sigma=6, sampling_rate=5, device=gpu_device)) as one, \
                contextlib.closing(sa.BiFMIndex.load(tmp_path / "parts.idx", device=gpu_device)) as back:
            assert one.info()["n_parts"] == 1 and back.info()["n_parts"] == 3 and back.info()["sampling_rate"] == 5
            for verify, locate_sa in MODES:
                for g in (one, parts, back):
                    g.set_mode(verify=verify, locate_sa=locate_sa)
                single = hits_as_rows(sa.search(one, pats, sch))
                assert np.array_equal(single, want), (verify, locate_sa)
                assert np.array_equal(hits_as_rows(sa.search(parts, pats, sch)), single), (verify, locate_sa)
                assert np.array_equal(hits_as_rows(sa.search(back, pats, sch)), single), (verify, locate_sa)


def assert_searches_like_oracle(gpu, sigma, pats, sch, edit, want):
    for verify, locate_sa in MODES:
        gpu.set_mode(verify=verify, locate_sa=locate_sa)
        assert np.array_equal(hits_as_rows(sa.search(gpu, pats, sch, edit=edit)), want), (verify, locate_sa)
    gpu.set_mode(verify=True, locate_sa=True)
    c = sa.search_packed_compact(gpu, sa.pack_reads(pats, sigma, pinned=True), sch, edit=edit, reverse=False)
    try:
        assert np.array_equal(hits_as_rows(c.to_hits()), want)
    finally:
        c.close()


@pytest.mark.parametrize("kmer", [None, "0"])
@pytest.mark.parametrize("rate", [16, 3])
@pytest.mark.parametrize("sigma,edit,m,k", DEGENERATE)
def test_degenerate_texts_searched(gpu_device, monkeypatch, sigma, edit, m, k, rate, kmer):
    """Records shorter than, as long as and barely longer than the pattern,
    and empty ones: the text-phase window is clamped at both ends at once.
    GPU == oracle in the four modes and through the packed call, with the
    default k-mer table and without one; oracle == brute force on the P-set."""
    if kmer is not None:
        monkeypatch.setenv("SAHARA_KMER", kmer)
    recs, pats = degenerate(sigma, edit, m, k)
    recs = list(recs)
    sch = sa.search_scheme("h2-k2", 0, k, m, hamming=not edit)
    want = hits_as_rows(O.Index.build(recs, sigma, rate).search(pats, sch, edit=edit)[0])
    assert pset(want) == pset(hits_as_rows(O.bruteforce(recs, pats, k, edit=edit)))
    assert len(np.unique(want[:, 1])) == sum(1 for r in recs if len(r) >= m - (k if edit else 0))
    with contextlib.closing(sa.BiFMIndex.build(recs, sigma=sigma, sampling_rate=rate, device=gpu_device)) as gpu:
        assert (gpu.info()["kmer_depth"] == 0) == (kmer == "0")
        assert_searches_like_oracle(gpu, sigma, pats, sch, edit, want)


@pytest.mark.parametrize("name", list(TINY))
def test_tiny_texts_searched(gpu_device, tmp_path, name):
    """The N = 2 index, and patterns longer than every record (no hit, no
    error) or as long as the whole text: built and loaded, the oracle's rows,
    whose P-set is the brute force's."""
    recs, m, k, pats = tiny(name)
    sch = sa.search_scheme("h2-k2", 0, k, m)
    ref = O.Index.build(recs, 6, 16)
    want = hits_as_rows(ref.search(pats, sch)[0])
    assert pset(want) == pset(hits_as_rows(O.bruteforce(recs, pats, k)))
    assert (len(want) > 0) == (name == "acg-c-m4")
    ref.write(tmp_path / "tiny.idx")
    with contextlib.closing(sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)) as gpu, \
            contextlib.closing(sa.BiFMIndex.load(tmp_path / "tiny.idx", device=gpu_device)) as back:
        assert_searches_like_oracle(gpu, 6, pats, sch, True, want)
        assert_searches_like_oracle(back, 6, pats, sch, True, want)


@pytest.mark.parametrize("bad", [0, 1 << 32, (1 << 32) + 16, (1 << 64) - 1])
def test_idx_with_an_impossible_rate_is_refused(gpu_device, bad):
    """parseIdx (host_util.cpp) refuses a rate of 0, which no LF walk satisfies,
    and one that does not fit the 32 bits it is kept in (2^32 + 16 would load
    as 16), before anything is uploaded."""
    case_id = "n1024-split"
    image = bytearray(oracle_image(case_id))
    at = rate_offset(6, len(records(case_id)))
    assert int.from_bytes(image[at:at + 8], "little") == 16
    image[at:at + 8] = bad.to_bytes(8, "little")
    with pytest.raises(sa.SaharaError, match="sampling rate"):
        sa.BiFMIndex.from_bytes(bytes(image), device=gpu_device)
    with loaded(case_id, gpu_device) as gpu:  # the unpatched image loads
        assert gpu.info()["sampling_rate"] == 16


def test_build_refuses_rate_zero(gpu_device):
    with pytest.raises(sa.SaharaError, match="sampling rate"):
        sa.BiFMIndex.build(list(records("n64")), sigma=6, sampling_rate=0, device=gpu_device)
