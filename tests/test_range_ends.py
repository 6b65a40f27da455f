"""The search calls at the ends of the range staging.cpp accepts: 5 to 15
errors (the 4-bit e of the scheme table, of the text kernel's node word and of
the compact hit records; fmStackCap's 152 levels and the text stack of 2k + 2),
16 besthits rounds, scheme tables of 255 searches and of exactly 15360 entries
(61 440 B of FM LDS, 94 208 B with SAHARA_FM_LDS_DEPTH=8; 122 880 B of text
table), patterns of 4096 to 16383 symbols, and the refusals just past each
limit.

Expected everywhere: the oracle's rows over its own index of the same records
(tests/range_cases.py; tests/test_range_inputs.py holds what each input is
for), compared as sorted (qid, seq_id, pos, e) rows, bit-exact."""
import numpy as np
import pytest

import align_model as am
import range_cases as R
import sahara_amd as sa
from helpers import hits_as_rows
from test_align_gpu import check_records
from test_text_variants import MODES, _reported_geometry

pytestmark = pytest.mark.gpu

ROUTES = ["search", "resident", "streamed"]


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    got = hits_as_rows(got)
    assert np.array_equal(got, want), what


def _run_routes(gpu, c, route):
    """search in the four (verify, locate_sa) modes | stage + run(count) + fetch
    | search_reads and the packed call with compact records (4-bit e)."""
    want, edit = c["want"], c["edit"]
    if route == "search":
        for mode in MODES:
            gpu.set_mode(verify=mode[0], locate_sa=mode[1])
            _same(sa.search(gpu, c["pats"], c["scheme"], edit=edit), want, ("search", mode))
            assert gpu.stats()["hits"] == len(want)
        gpu.set_mode(verify=True, locate_sa=True)
    elif route == "resident":
        gpu.stage(c["pats"], c["scheme"], edit=edit)
        assert gpu.run(count=True) == len(want)
        st = gpu.stats()
        assert st["hits"] == len(want)
        _same(gpu.fetch(), want, "stage/run(count)/fetch")
        return st
    else:
        _same(sa.search_reads(gpu, c["reads"], c["scheme"], edit=edit, reverse=c["reverse"]), want, "search_reads")
        pk = sa.pack_reads(c["reads"], c["sigma"], pinned=True)
        ch = sa.search_packed_compact(gpu, pk, c["scheme"], edit=edit, reverse=c["reverse"])
        try:
            assert gpu.info()["n_parts"] == 1
            _same(ch.to_hits(), want, "search_packed_compact")
        finally:
            ch.close()
    return gpu.stats()


def _case_through(gpu_device, c, route):
    gpu = sa.BiFMIndex.build(c["recs"], sigma=c["sigma"], device=gpu_device)
    try:
        return _run_routes(gpu, c, route)
    finally:
        gpu.close()


# ------------------------------------------- a. Hamming up to 15 errors ----

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.HAMMING))
def test_hamming_up_to_15_errors(gpu_device, name, route):
    st = _case_through(gpu_device, R.hamming(name), route)
    if route == "resident":  # the text kernel took part: its node word's e runs to k
        assert st["conversions"] > 0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("variant", ["rc", "batch7"])
def test_pigeon_k15_interleaved_and_in_small_batches(gpu_device, monkeypatch, variant, route):
    if variant == "batch7":
        monkeypatch.setenv("SAHARA_BATCH", "7")
    st = _case_through(gpu_device, R.hamming("pigeon-k15", variant == "rc"), route)
    if variant == "batch7":
        assert st["batches"] >= 100 // 7


# ------------------------- b. edit distance, all-mode, k = 5 to 8 ----------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.EDIT))
def test_edit_all_mode_k5_to_k8(gpu_device, name, route):
    _case_through(gpu_device, R.edit(name), route)


# ------------------- c. edit distance up to 15 errors: staircase schemes ----

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(R.STAIRCASE))
def test_edit_staircase_to_15_errors(gpu_device, name, route):
    st = _case_through(gpu_device, R.staircase(name), route)
    if route == "resident":
        assert st["conversions"] > 0


# ------------------------------------------ d. besthits over 16 rounds ----

@pytest.mark.parametrize("batch", [None, "7"])
def test_besthits_over_16_rounds(gpu_device, monkeypatch, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = R.best16()
    want, schemes = c["want"], c["schemes"]
    gpu = sa.BiFMIndex.build(c["recs"], sigma=c["sigma"], device=gpu_device)
    try:
        _same(sa.search_best(gpu, c["pats"], schemes), want, "search_best")
        assert gpu.stats()["best_rounds"] == 16
        _same(sa.search_best_reads(gpu, c["reads"], schemes, reverse=False), want, "search_best_reads")
        assert gpu.stats()["best_rounds"] == 16
        # the rounds once more over what the call left staged, counting: queries found in a round skip the later ones
        assert gpu.run(count=True) == len(want)
        st = gpu.stats()
        assert st["best_rounds"] == 16 and st["best_skipped"] > 0 and st["hits"] == len(want)
        _same(gpu.fetch(), want, "count-mode rounds")
        pk = sa.pack_reads(c["reads"], c["sigma"], pinned=True)
        _same(sa.search_best_packed(gpu, pk, schemes, reverse=False), want, "search_best_packed")
        ch = sa.search_best_packed_compact(gpu, pk, schemes, reverse=False)
        try:
            _same(ch.to_hits(), want, "search_best_packed_compact")
        finally:
            ch.close()
        st = gpu.stats()
        assert st["best_rounds"] == 16
        if batch:
            assert st["batches"] >= 32 // 7
    finally:
        gpu.close()


# ------------------------------------ e. the scheme table at its limits ----

@pytest.mark.parametrize("depth", ["0", "8"])
@pytest.mark.parametrize("verify", [True, False], ids=["text", "fm"])
@pytest.mark.parametrize("name", list(R.TABLE))
def test_scheme_table_at_its_limits(gpu_device, capfd, monkeypatch, name, verify, depth):
    """A launch the runtime refuses comes back as a SaharaError and fails this
    test: staging accepted the shape. The text phase is asserted to have run
    only where the library's own report gives it a workgroup per CU."""
    c = R.table(name)
    nsearch, m = R.TABLE[name]
    monkeypatch.setenv("SAHARA_FM_LDS_DEPTH", depth)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=c["sigma"], device=gpu_device)
    try:
        gpu.set_mode(verify=verify, locate_sa=verify)
        gpu.stage(c["pats"], c["scheme"], edit=False)
        _, lds, bpc = _reported_geometry(gpu, capfd, monkeypatch, f"{name} verify {verify} depth {depth}")
        print(f"{name}: FM table {nsearch * m * 4} B, FM LDS {nsearch * m * 4 + int(depth) * 4096} B, text LDS {lds} B")
        # (pass_plan.h textGeometry: the table of two words per entry, then 256 lanes of window, pattern and stack)
        assert 2 * nsearch * m * 4 < lds <= 160 * 1024
        _same(sa.search(gpu, c["pats"], c["scheme"], edit=False), c["want"], "search")
        st = _run_routes(gpu, c, "resident")
        if verify and bpc >= 1:
            assert st["conversions"] > 0
        if not verify:
            assert st["conversions"] == 0
        _run_routes(gpu, c, "streamed")
    finally:
        gpu.close()


# --------------------------------------------------- f. long patterns ----

def _text_and_starts(recs):
    return am.concat_text(recs), np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])]).astype(np.int64)


@pytest.mark.parametrize("name", list(R.LONG))
def test_long_patterns(gpu_device, name):
    """One search, FM phase only (the text phase is off above 2047 symbols);
    then the hits aligned on the device against tests/align_model.py."""
    c = R.long(name)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=c["sigma"], device=gpu_device)
    try:
        for mode in ((True, True), (False, False)):
            gpu.set_mode(verify=mode[0], locate_sa=mode[1])
            hits = sa.search(gpu, c["pats"], c["scheme"], edit=c["edit"])
            _same(hits, c["want"], ("search", mode))
        gpu.set_mode(verify=True, locate_sa=True)
        st = _run_routes(gpu, c, "resident")
        assert st["conversions"] == 0
        _run_routes(gpu, c, "streamed")
        T, starts = _text_and_starts(c["recs"])
        got = sa.align(gpu, c["pats"], hits, edit=c["edit"], max_err=2)
        check_records(got, c["pats"], hits, T, starts, 2, c["edit"], ("range", name))
        assert (got["err"] <= hits["err"]).all()
    finally:
        gpu.close()


@pytest.mark.parametrize("edit", [True, False], ids=["edit", "hamming"])
def test_align_at_the_longest_pattern(gpu_device, edit):
    """16383 symbols, 0..8 substitutions, max_err = 8, at positions known by
    construction: no search."""
    recs, reads, places, subs = R.align_longest()
    hits = np.zeros(len(reads), sa.HIT_DTYPE)
    hits["qid"] = np.arange(len(reads))
    hits["seq_id"] = [s for s, _ in places]
    hits["pos"] = [t for _, t in places]
    gpu = sa.BiFMIndex.build(recs, sigma=6, device=gpu_device)
    try:
        T, starts = _text_and_starts(recs)
        got = sa.align(gpu, reads, hits, edit=edit, max_err=8)
        check_records(got, reads, hits, T, starts, 8, edit, ("longest", edit))
        assert got["err"].tolist() == subs and (got["ref_len"] == R.ALIGN_LONGEST).all()
        with pytest.raises(sa.SaharaError, match="pattern length out of range"):  # one symbol more: refused on the host
            sa.align(gpu, np.ones((1, R.ALIGN_LONGEST + 1), np.uint8), hits[:1], edit=edit, max_err=8)
    finally:
        gpu.close()


# --------------------------------- g. refusals, just past each limit ----

def _flat_scheme(pi):
    pi = np.asarray([pi], np.uint32)
    return pi, np.zeros_like(pi), np.zeros_like(pi)


def _refusals():
    """[(id, message, reads, scheme)]: each just past one limit of staging.cpp."""
    good = R.hamming("h2-k2-k8")
    reads, (pi, l, u) = good["reads"], good["scheme"]
    u16, l_over = u.copy(), l.copy()
    u16[0, -1] = 16
    l_over[1, 5] = u[1, 5] + 1
    rec = good["recs"][0]
    of_len = lambda m: np.ascontiguousarray(np.stack([rec[i:i + m] for i in range(0, 8)]))
    long_read = np.ascontiguousarray(np.resize(rec, 65536)[None, :])
    return [
        ("u16", "l <= u <= 15", reads, (pi, l, u16)),
        ("l-over-u", "l <= u <= 15", reads, (pi, l_over, u)),
        ("pi-123-m3", "pi out of range", of_len(3), _flat_scheme([1, 2, 3])),
        ("pi-2134-m4", "pi out of range", of_len(4), _flat_scheme([2, 1, 3, 4])),  # [2, 1, 0, 3, 4] less one step
        ("pi-first-m4", "pi out of range", of_len(4), _flat_scheme([4, 3, 2, 1])),
        ("pi-gap", "connected order", of_len(3), _flat_scheme([0, 2, 1])),
        ("256x60", "255 searches", of_len(60), R.filled_scheme(256, 60)),
        ("241x64", "too large for LDS", of_len(64), R.filled_scheme(241, 64)),
        ("m65536", "length out of range", long_read, _flat_scheme(np.arange(65536))),
    ]


REFUSALS = ["u16", "l-over-u", "pi-123-m3", "pi-2134-m4", "pi-first-m4", "pi-gap", "256x60", "241x64", "m65536"]


@pytest.fixture(scope="module")
def refusal_index(gpu_device):
    good = R.hamming("h2-k2-k8")
    gpu = sa.BiFMIndex.build(good["recs"], sigma=good["sigma"], device=gpu_device)
    yield gpu
    gpu.close()


@pytest.mark.parametrize("which", REFUSALS)
def test_refusals_just_past_each_limit(refusal_index, which):
    """Refused on the host, before any launch, by search and by the streamed
    call alike; the same context then answers a valid call with the oracle's
    rows. (pi-123-m3 and pi-2134-m4 reached the kernels before packSchemeTable
    bounded every pi by m, not the first alone: they read pattern position m of
    m symbols.)"""
    gpu, good = refusal_index, R.hamming("h2-k2-k8")
    table = {r[0]: r for r in _refusals()}
    assert list(table) == REFUSALS
    _, message, reads, scheme = table[which]
    with pytest.raises(sa.SaharaError, match=message):
        sa.search(gpu, reads, scheme, edit=False)
    _same(sa.search(gpu, good["pats"], good["scheme"], edit=False), good["want"], "search after a refusal")
    with pytest.raises(sa.SaharaError, match=message):
        sa.search_reads(gpu, reads, scheme, edit=False, reverse=False)
    _same(sa.search_reads(gpu, good["reads"], good["scheme"], edit=False, reverse=False), good["want"],
          "search_reads after a refusal")
