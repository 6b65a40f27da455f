"""Every compiled variant of the text kernel (kSearchTextBatch<EDIT, COUNT,
SHAPE>: search_text.hip), the read lengths at which the text geometry
changes (pass_plan.h textGeometry, search_text.hip textShapeOf), the edges of the
seed stage (kSeedItems, seedCode, stageSchemes' kmerStart) and the scheduling
knobs of pass_plan.h away from their defaults.

Expected everywhere: the oracle's hits over its own index of the records,
compared as sorted (qid, seq_id, pos, e) rows, bit-exact. Which kernel shape
ran is read from the library's own report (pass.cpp makePlan under
SAHARA_DUMP_COUNTERS), never restated here: a case that lands on another
shape than it names fails. tests/pass_plan_check.cpp holds the same geometry
worked out by hand, on the host."""
import functools
import re

import numpy as np
import pytest

import oracle as O
import sahara_amd as sa
from helpers import hits_as_rows, mutate_reads, random_records, substituted_reads

pytestmark = pytest.mark.gpu

MODES = [(True, True), (False, False), (True, False), (False, True)]  # (verify, locate_sa)
N_RANK = 4  # dna5's N


# ---------------------------------------------------------------- inputs ----

def _with_record_ends(body, recs, m):
    """The reads, then every record's first and last m symbols."""
    ends = [r[:m] for r in recs] + [r[-m:] for r in recs]
    return np.ascontiguousarray(np.vstack([body, np.stack(ends)]))


def _check_input(want, recs, m, k):
    """What a case's own input must hold before the GPU is looked at: hits of
    every error count, one at the start of a record, one reaching its end."""
    assert set(want[:, 3].tolist()) == set(range(k + 1)), sorted(set(want[:, 3].tolist()))
    assert (want[:, 2] == 0).any()
    lens = np.array([len(r) for r in recs], np.uint64)
    assert (want[:, 2] + np.uint64(m) >= lens[want[:, 1].astype(np.int64)]).any()


@functools.lru_cache(maxsize=None)
def _case(sigma, edit, m, k, gen="h2-k2"):
    """Records, reads, patterns, scheme and the oracle's rows of one (m, k)."""
    rng = np.random.default_rng(1000 * m + 10 * k + sigma + (1 if edit else 0))
    lengths = [int(x) for x in np.linspace(m + k + 1, 3 * m, 12)] + [20000, 9000]
    recs = random_records(rng, lengths, sigma, with_n=True, repeats=True)
    n = 100 if m > 300 else 200
    body = mutate_reads(rng, recs, n, m, k, sigma) if edit else substituted_reads(rng, recs, n, m, k, sigma)
    reads = _with_record_ends(body, recs, m)
    pats = sa.interleave_rc(reads, sigma)
    scheme = sa.search_scheme(gen, 0, k, m, hamming=not edit)
    want = hits_as_rows(O.Index.build(recs, sigma, 16).search(pats, scheme, edit=edit, nthreads=8)[0])
    _check_input(want, recs, m, k)
    return dict(sigma=sigma, edit=edit, m=m, k=k, recs=recs, reads=reads, pats=pats, scheme=scheme, want=want)


# ---------------------------------------------- the library's own report ----

_GEOMETRY = re.compile(r"text geometry: shape (\d+) lds (\d+) blocks/CU (-?\d+) \(alone (-?\d+)\) serial (\d)")


def _reported_geometry(gpu, capfd, monkeypatch, label, count=False):
    """One pass over the staged patterns under SAHARA_DUMP_COUNTERS, for
    makePlan's report alone: (shape, lds, blocks/CU). The variable is unset
    again before anything is compared (the knobs are read per pass)."""
    capfd.readouterr()
    monkeypatch.setenv("SAHARA_DUMP_COUNTERS", "1")
    try:
        gpu.run(count=count)
    finally:
        monkeypatch.delenv("SAHARA_DUMP_COUNTERS")
    err = capfd.readouterr().err
    found = _GEOMETRY.findall(err)
    assert found, err[-2000:]
    shape, lds, bpc = int(found[0][0]), int(found[0][1]), int(found[0][2])
    assert all(int(f[0]) == shape and int(f[1]) == lds for f in found), found  # (a re-run after an overflow plans again)
    print(f"{label}: shape {shape} lds {lds} blocks/CU {bpc} (alone {found[0][3]})")
    return shape, lds, bpc


def _same(got, want, what):
    got = hits_as_rows(got)
    assert len(got) == len(want) and np.array_equal(got, want), what


def _count_run(gpu, c, mode):
    """stage + run(count=True) + fetch in one execution mode -> the run's stats."""
    gpu.set_mode(verify=mode[0], locate_sa=mode[1])
    gpu.stage(c["pats"], c["scheme"], edit=c["edit"])
    n = gpu.run(count=True)
    st = gpu.stats()
    assert n == len(c["want"]) == st["hits"], ("count mode", mode)
    _same(gpu.fetch(), c["want"], ("count mode fetch", mode))
    return st


# ------------------------------------------------------ a. variant matrix ----

SHAPE_AT = {0: (60, 2), 1: (100, 2), 2: (250, 3)}


@pytest.mark.parametrize("shape", [0, 1, 2])
@pytest.mark.parametrize("edit", [True, False], ids=["edit", "hamming"])
@pytest.mark.parametrize("sigma", [6, 5])
def test_variant_matrix(gpu_device, capfd, monkeypatch, sigma, edit, shape):
    """Both alphabets x both metrics x the three kernel shapes, each through
    every entry point: the four execution modes of search, the count-mode
    kernels with and without the text phase, the streamed calls from ranks
    and from packed reads in page-locked memory."""
    m, k = SHAPE_AT[shape]
    c = _case(sigma, edit, m, k)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=sigma, device=gpu_device)
    try:
        gpu.stage(c["pats"], c["scheme"], edit=edit)
        got_shape, _, bpc = _reported_geometry(gpu, capfd, monkeypatch, f"sigma {sigma} edit {edit} m {m} k {k}")
        assert got_shape == shape and bpc >= 1
        # (the count-mode kernels are picked by the same plan; its own report says so)
        assert _reported_geometry(gpu, capfd, monkeypatch, "  in count mode", count=True)[0] == shape
        for mode in MODES:
            gpu.set_mode(verify=mode[0], locate_sa=mode[1])
            _same(sa.search(gpu, c["pats"], c["scheme"], edit=edit), c["want"], ("search", mode))
        assert _count_run(gpu, c, (True, True))["conversions"] > 0
        assert _count_run(gpu, c, (False, False))["conversions"] == 0
        gpu.set_mode(verify=True, locate_sa=True)
        _same(sa.search_reads(gpu, c["reads"], c["scheme"], edit=edit), c["want"], "search_reads")
        pk = sa.pack_reads(c["reads"], sigma, pinned=True)
        ch = sa.search_packed_compact(gpu, pk, c["scheme"], edit=edit)
        _same(ch.to_hits(), c["want"], "search_packed_compact")
        ch.close()
    finally:
        gpu.close()


# ------------------------------------------------------ b. geometry edges ----

EDGES = [  # m, k, edit, the shape that must run
    (96, 2, True, 0), (97, 2, True, 1),      # pattern blocks 3 -> 4
    (124, 2, True, 1), (125, 2, True, 0),    # m + 2k = 128 fills shape 1's window; 129: 5 blocks
    (128, 0, True, 1), (126, 1, False, 1),   # window = pattern = 4 full blocks; m + 2k = 128, Hamming
    (220, 2, True, 0), (221, 2, True, 0),    # exact 7-block window (8 loads) -> aligned 8-block window
    (225, 0, True, 0), (225, 1, False, 2),   # aligned 8 blocks -> shape 2's lower end
    (251, 3, True, 2), (252, 3, True, 0),    # shape 2's upper end (257) -> 10 window blocks
    (256, 0, True, 2), (257, 0, True, 0),    # pattern 8 full blocks -> 9 blocks in two copy rounds
]


def _edge_runs(gpu, c):
    """search and a count-mode run with the text phase and without it -> the
    count-mode stats of the run with it."""
    st = None
    for mode in ((False, False), (True, True)):
        gpu.set_mode(verify=mode[0], locate_sa=mode[1])
        _same(sa.search(gpu, c["pats"], c["scheme"], edit=c["edit"]), c["want"], ("search", mode))
        st = _count_run(gpu, c, mode)
    return st


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[f"m{m}-k{k}-{'edit' if e else 'hamming'}" for m, k, e, _ in EDGES])
def test_geometry_edges(gpu_device, capfd, monkeypatch, i):
    m, k, edit, shape = EDGES[i]
    sigma = 6 if i % 2 == 0 else 5  # both alphabets see every shape
    c = _case(sigma, edit, m, k)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=sigma, device=gpu_device)
    try:
        gpu.stage(c["pats"], c["scheme"], edit=edit)
        got_shape, _, bpc = _reported_geometry(gpu, capfd, monkeypatch, f"sigma {sigma} edit {edit} m {m} k {k}")
        assert got_shape == shape and bpc >= 1
        assert _edge_runs(gpu, c)["conversions"] > 0
    finally:
        gpu.close()


def test_pigeon_hamming_at_shape_2(gpu_device, capfd, monkeypatch):
    """pigeon k = 3 at m = 250: four searches, Hamming, dna4."""
    c = _case(5, False, 250, 3, gen="pigeon")
    gpu = sa.BiFMIndex.build(c["recs"], sigma=5, device=gpu_device)
    try:
        gpu.stage(c["pats"], c["scheme"], edit=False)
        got_shape, _, bpc = _reported_geometry(gpu, capfd, monkeypatch, "sigma 5 pigeon hamming m 250 k 3")
        assert got_shape == 2 and bpc >= 1
        assert _edge_runs(gpu, c)["conversions"] > 0
    finally:
        gpu.close()


@pytest.mark.parametrize("m,sigma", [(640, 6), (672, 5), (673, 6)])
def test_around_the_lds_limit(gpu_device, capfd, monkeypatch, m, sigma):
    """h2-k2, k = 2, three searches: the plan's formula gives 156 672 B at 640,
    163 584 B at 672 (256 B below the 160 KB; the kernel holds 64 B of static
    LDS besides) and 166 680 B at 673, which runs FM only. The hits are the
    oracle's at all three; the text phase runs at 640 and does not at 673.
    What the runtime grants at 672 is reported, not asserted."""
    c = _case(sigma, True, m, 2)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=sigma, device=gpu_device)
    try:
        gpu.stage(c["pats"], c["scheme"], edit=True)
        shape, lds, bpc = _reported_geometry(gpu, capfd, monkeypatch, f"sigma {sigma} edit True m {m} k 2")
        assert shape == 0
        st = _edge_runs(gpu, c)
        print(f"m {m}: conversions {st['conversions']} text_grid {st['text_grid']}")
        if m == 640:
            assert lds <= 160 * 1024 and bpc >= 1 and st["conversions"] > 0
        if m == 673:
            assert lds > 160 * 1024 and bpc == 0 and st["conversions"] == 0
    finally:
        gpu.close()


# ------------------------------------- c. besthits at the bench's shape ----

@functools.lru_cache(maxsize=None)
def _best_case(sigma, m):
    rng = np.random.default_rng(31 * m + sigma)
    recs = random_records(rng, [25000, 8000], sigma, with_n=True, repeats=True)
    reads = np.concatenate([mutate_reads(rng, recs, 100, m, e, sigma) for e in range(3)])  # 0, 1, 2 errors by thirds
    reads = np.ascontiguousarray(reads[rng.permutation(len(reads))])
    pats = sa.interleave_rc(reads, sigma)
    schemes = [sa.search_scheme("h2-k2", j, j, m) for j in range(3)]
    want = hits_as_rows(O.search_best(O.Index.build(recs, sigma, 16), pats, schemes, nthreads=8))
    # every round reports (rows of its error count) and skips (queries found before it)
    assert set(want[:, 3].tolist()) == {0, 1, 2}
    return dict(sigma=sigma, recs=recs, reads=reads, pats=pats, schemes=schemes, want=want)


@pytest.mark.parametrize("batch", ["97", None])
@pytest.mark.parametrize("sigma", [6, 5])
@pytest.mark.parametrize("m", [100, 124])
def test_besthits_rounds_at_shape_1(gpu_device, capfd, monkeypatch, m, sigma, batch):
    if batch:
        monkeypatch.setenv("SAHARA_BATCH", batch)
    c = _best_case(sigma, m)
    gpu = sa.BiFMIndex.build(c["recs"], sigma=sigma, device=gpu_device)
    try:
        _same(sa.search_best(gpu, c["pats"], c["schemes"]), c["want"], "search_best")
        assert gpu.stats()["best_rounds"] == 3
        _same(sa.search_best_reads(gpu, c["reads"], c["schemes"]), c["want"], "search_best_reads")
        assert gpu.stats()["best_rounds"] == 3
        # the rounds' plan, over the patterns and schemes the call left staged
        shape, _, bpc = _reported_geometry(gpu, capfd, monkeypatch, f"besthits sigma {sigma} m {m} batch {batch}")
        assert shape == 1 and bpc >= 1 and gpu.stats()["best_rounds"] == 3
        assert gpu.run(count=True) == len(c["want"])
        st = gpu.stats()
        assert st["best_rounds"] == 3 and st["best_skipped"] > 0 and st["conversions"] > 0
        _same(gpu.fetch(), c["want"], "count-mode rounds")
        pk = sa.pack_reads(c["reads"], sigma, pinned=True)
        ch = sa.search_best_packed_compact(gpu, pk, c["schemes"])
        _same(ch.to_hits(), c["want"], "search_best_packed_compact")
        ch.close()
    finally:
        gpu.close()


# ------------------------------------------------- d. seed-stage edges ----

@functools.lru_cache(maxsize=None)
def _seed_text(sigma):
    """60 000 + 20 000 symbols with repeats, and 400 symbols of record 0 once
    more in record 1: k-mers of any depth with several rows."""
    rng = np.random.default_rng(400 + sigma)
    recs = random_records(rng, [60000, 20000], sigma, with_n=True, repeats=True)
    recs[1][5000:5400] = recs[0][1000:1400]
    return recs


def _kmer_counts(recs, K, sigma):
    """code -> occurrences of every K-mer over A C G T in the records."""
    digit = np.full(8, -1, np.int64)
    digit[[1, 2, 3, 5 if sigma == 6 else 4]] = [0, 1, 2, 3]
    weights = 4 ** np.arange(K - 1, -1, -1, dtype=np.int64)
    codes = []
    for r in recs:
        w = np.lib.stride_tricks.sliding_window_view(digit[r], K)
        codes.append((w[(w >= 0).all(axis=1)] * weights).sum(axis=1))
    keys, n = np.unique(np.concatenate(codes), return_counts=True)
    return digit, weights, dict(zip(keys.tolist(), n.tolist()))


def _seed_expectation(recs, pats, scheme, K, sigma):
    """The seed stage's rules (search_fm.hip kSeedItems) over this input: (items
    it keeps, items that become text tasks). A search whose first K steps admit
    no error starts from the K-mer at the least of their pattern positions: an
    item whose K-mer is absent from the text is dropped, one whose K-mer has a
    single row (and is shorter than the pattern) becomes a task; an N in the
    K-mer, or a search that may err within K steps, starts at the root."""
    pi, _, u = scheme
    m = pats.shape[1]
    digit, weights, counts = _kmer_counts(recs, K, sigma)
    kept = tasks = 0
    for s in range(pi.shape[0]):
        if K > m or u[s, :K].any():
            kept += len(pats)
            continue
        lo = int(pi[s, :K].min())
        d = digit[pats[:, lo:lo + K]]
        clean = (d >= 0).all(axis=1)
        rows = np.array([counts.get(int(x), 0) for x in (d[clean] * weights).sum(axis=1)])
        kept += int((~clean).sum()) + int((rows > 0).sum())
        if K < m:
            tasks += int((rows == 1).sum())
    return kept, tasks


@functools.lru_cache(maxsize=None)
def _seed_case(sigma, m, k, gen, planted_n=0):
    """Reads from all over the text and 40 from the stretch that occurs twice;
    planted_n = K: an N inside the first K steps of a search, search by search."""
    recs = _seed_text(sigma)
    rng = np.random.default_rng(7 * m + k + sigma + len(gen))
    twice = [recs[0][1000:1400]]
    body = np.vstack([mutate_reads(rng, recs, 200, m, k, sigma), mutate_reads(rng, twice, 40, m, k, sigma)])
    reads = _with_record_ends(body, recs, m)
    scheme = sa.search_scheme(gen, 0, k, m)
    if planted_n:
        assert sigma == 6
        pi = scheme[0]
        for i, r in enumerate(reads):
            r[pi[i % len(pi), rng.integers(planted_n)]] = N_RANK
    pats = sa.interleave_rc(reads, sigma)
    want = hits_as_rows(O.Index.build(recs, sigma, 16).search(pats, scheme, edit=True, nthreads=8)[0])
    assert len(want) > len(pats) // 4 and (want[:, 2] == 0).any()
    return dict(sigma=sigma, edit=True, m=m, k=k, recs=recs, reads=reads, pats=pats, scheme=scheme, want=want)


_SEED_GPU = {}


def _seed_index(sigma, depth, device, monkeypatch):
    """One index per (alphabet, depth), SAHARA_KMER set while it is built."""
    if (sigma, depth) not in _SEED_GPU:
        monkeypatch.setenv("SAHARA_KMER", str(depth))
        _SEED_GPU[sigma, depth] = sa.BiFMIndex.build(_seed_text(sigma), sigma=sigma, device=device)
        monkeypatch.delenv("SAHARA_KMER")
    gpu = _SEED_GPU[sigma, depth]
    assert gpu.info()["kmer_depth"] == depth
    return gpu


SEED_CASES = [  # depth, m, k, generator, N planted, tasks expected
    (12, 12, 0, "h2-k2", False, False),  # the pattern ends where the table does: its leaf comes from the FM kernel
    (12, 13, 0, "h2-k2", False, True),   # one symbol more
    (12, 10, 0, "h2-k2", False, False),  # shorter than the table is deep: seeds start at the root
    (8, 23, 2, "h2-k2", False, True),    # first parts of K - 1 and K symbols
    (8, 24, 2, "h2-k2", False, True),    # of K
    (8, 25, 2, "h2-k2", False, True),    # of K and K + 1
    (8, 24, 2, "pigeon", False, True),
    (8, 24, 2, "01*0", False, True),
    (8, 24, 2, "h2-k2", True, True),     # an N in the K-mer: that item falls back to the root
]


SEED_PARAMS = [(sigma,) + case for case in SEED_CASES for sigma in ((6,) if case[4] else (6, 5))]  # (dna4 has no N)


@pytest.mark.parametrize("sigma,depth,m,k,gen,planted,expect_tasks", SEED_PARAMS,
                         ids=[f"dna{s - 1}-K{d}-m{m}-k{k}-{g}{'-N' if p else ''}" for s, d, m, k, g, p, _ in SEED_PARAMS])
def test_seed_stage_edges(gpu_device, monkeypatch, sigma, depth, m, k, gen, planted, expect_tasks):
    c = _seed_case(sigma, m, k, gen, depth if planted else 0)
    kept, tasks = _seed_expectation(c["recs"], c["pats"], c["scheme"], depth, sigma)
    print(f"K {depth} m {m} k {k} {gen}: {len(c['pats']) * len(c['scheme'][0])} items, kept {kept}, single-row tasks {tasks}")
    assert (0 < tasks < kept) if expect_tasks else tasks == 0
    if planted:
        assert (c["pats"] == N_RANK).any(axis=1).all()
    gpu = _seed_index(sigma, depth, gpu_device, monkeypatch)
    try:
        st = _count_run(gpu, c, (True, True))
        print(f"text_pos_tasks {st['text_pos_tasks']} conversions {st['conversions']}")
        assert st["text_pos_tasks"] == tasks and st["conversions"] >= tasks
        if expect_tasks:
            assert 0 < st["text_pos_tasks"] < kept
        _same(sa.search(gpu, c["pats"], c["scheme"]), c["want"], "search")
        for knob in ("SAHARA_SEED_TASKS", "SAHARA_KMER_POS"):
            monkeypatch.setenv(knob, "0")
            _same(sa.search(gpu, c["pats"], c["scheme"]), c["want"], knob)
            assert _count_run(gpu, c, (True, True))["text_pos_tasks"] == 0, knob
            monkeypatch.delenv(knob)
        gpu.set_mode(verify=False, locate_sa=False)
        _same(sa.search(gpu, c["pats"], c["scheme"]), c["want"], "reference execution")
    finally:
        gpu.set_mode(verify=True, locate_sa=True)


# ------------------------------------------------- e. scheduling knobs ----

@functools.lru_cache(maxsize=None)
def _knob_case():
    """Repeat-rich text, k = 3, m = 80, h2-k3: deep subtrees, and with
    SAHARA_BATCH=333 several small batches."""
    rng = np.random.default_rng(79)
    recs = random_records(rng, [30000, 12000], 6, repeats=True)
    reads = mutate_reads(rng, recs, 400, 80, 3, 6)
    pats = sa.interleave_rc(reads, 6)
    scheme = sa.search_scheme("h2-k3", 0, 3, 80)
    assert len(scheme[0]) == 7  # (pass_plan_check.cpp: fmLdsBytes of seven searches)
    want = hits_as_rows(O.Index.build(recs, 6, 16).search(pats, scheme, edit=True, nthreads=8)[0])
    return dict(sigma=6, edit=True, recs=recs, reads=reads, pats=pats, scheme=scheme, want=want)


_KNOB_GPU = []

KNOBS = [  # variable, value, (verify, locate_sa)
    ("SAHARA_TEXT_STEPS", "1", (True, True)), ("SAHARA_TEXT_STEPS", "4", (True, True)),
    ("SAHARA_REFILL_AT", "1", (True, True)), ("SAHARA_REFILL_AT", "64", (True, True)),
    ("SAHARA_KMER_POS", "0", (True, True)),
    ("SAHARA_FM_LDS_DEPTH", "1", (True, True)), ("SAHARA_FM_LDS_DEPTH", "8", (True, True)),
    ("SAHARA_FM_LDS_DEPTH", "0", (False, False)), ("SAHARA_FM_LDS_DEPTH", "8", (False, False)),
    ("SAHARA_FM_BPC", "1", (True, True)), ("SAHARA_FM_BPC", "1", (False, False)),
    ("SAHARA_TEXT_BPC", "1", (True, True)),
    ("SAHARA_POLL_US", "0", (True, True)),
    (None, None, (True, True)), (None, None, (False, False)),  # the defaults beside them
]


@pytest.mark.parametrize("knob,value,mode", KNOBS,
                         ids=[f"{(n or 'defaults').replace('SAHARA_', '')}{'=' + v if v else ''}-{'text' if md[0] else 'fm'}"
                              for n, v, md in KNOBS])
def test_scheduling_knobs(gpu_device, monkeypatch, knob, value, mode):
    """One variable away from its default at a time: the oracle's rows and the
    same hit count from search, from the device-resident run and from the
    streamed call over the reads."""
    c = _knob_case()
    if not _KNOB_GPU:
        _KNOB_GPU.append(sa.BiFMIndex.build(c["recs"], sigma=6, device=gpu_device))
    gpu = _KNOB_GPU[0]
    monkeypatch.setenv("SAHARA_BATCH", "333")
    if knob:
        monkeypatch.setenv(knob, value)
    try:
        gpu.set_mode(verify=mode[0], locate_sa=mode[1])
        _same(sa.search(gpu, c["pats"], c["scheme"]), c["want"], "search")
        assert gpu.stats()["hits"] == len(c["want"])
        gpu.stage(c["pats"], c["scheme"])
        assert gpu.run() == len(c["want"]) == gpu.stats()["hits"]
        _same(gpu.fetch(), c["want"], "stage/run/fetch")
        st = gpu.stats()
        assert st["batches"] > 1 and (st["text_grid"] > 0) == mode[0]
        if knob in ("SAHARA_FM_BPC", "SAHARA_TEXT_BPC"):  # one workgroup per CU: the grid shrinks
            grid = "search_grid" if knob == "SAHARA_FM_BPC" else "text_grid"
            monkeypatch.delenv(knob)
            gpu.run()
            by_default = gpu.stats()[grid]
            monkeypatch.setenv(knob, value)
            if (knob, mode[0]) == ("SAHARA_FM_BPC", True):  # beside the text phase the FM phase has one per CU anyway
                assert st[grid] == by_default
            else:
                assert 0 < st[grid] < by_default
        _same(sa.search_reads(gpu, c["reads"], c["scheme"]), c["want"], "search_reads")
        assert gpu.stats()["hits"] == len(c["want"])
    finally:
        gpu.set_mode(verify=True, locate_sa=True)
