"""The CPU restatement's index (oracle/oracle.cpp: prefix doubling) against the
from-scratch model of tests/index_model.py (a naive sort of the suffixes), over
the whole case table of tests/index_cases.py: every sampling rate, every size
edge, LCPs on the doubling steps, homopolymers, identical and empty records.
The GPU tests of tests/test_index_edges.py compare the device with the same
model; here the oracle is held to it without a GPU, and its .idx round trip
keeps the sampling rate. The degenerate search inputs of the GPU tests are
pinned to the brute-force DP here as well."""
import numpy as np
import pytest

import oracle as O
from helpers import hits_as_rows, pset
from index_cases import (CASES, DEGENERATE, LOCATE_CASES, RATES, TINY, degenerate, locate_inputs, oracle_index,
                         rate_offset, records, reference, tiny)
from index_model import model

IDS = [c.id for c in CASES]


def test_case_table_counts():
    kinds = [c.kind for c in CASES]
    assert (kinds.count("rate"), kinds.count("size"), kinds.count("doubling")) == (13, 32, 31)


@pytest.mark.parametrize("case_id", IDS)
def test_oracle_index_equals_model(case_id):
    want = reference(case_id)
    idx = oracle_index(case_id)
    assert idx.n == want["n"]
    got = idx.export()
    for key in ("sa", "bwt_f", "bwt_r", "sampled", "samples"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["C"][: len(want["C"])], want["C"])
    assert int(O.lib().orc_nsamples(idx.h)) == want["n_samples"]


def test_model_on_a_text_worked_by_hand():
    """[AC, A] = A C $ A $: suffixes in order $ (4), $A$ (2), A$ (3), AC$A$ (0), C$A$ (1)."""
    got = model([[1, 2], [1]], 6, 2)
    assert got["text"].tolist() == [1, 2, 0, 1, 0]
    assert got["sa"].tolist() == [4, 2, 3, 0, 1]
    assert got["bwt_f"].tolist() == [1, 2, 0, 0, 1]
    assert got["C"].tolist() == [0, 2, 4, 5, 5, 5, 5]
    # in-record offsets 0 1 2 | 0 1: rows of positions 4, 2 (delimiters), 3, 0 (offset 0); not 1
    assert got["sampled"].tolist() == [0b01111] and got["samples"].tolist() == [4, 2, 3, 0]
    # reverse text C A $ A $: $ (4), $A$ (2), A$ (3), A$A$ (1), CA$A$ (0)
    assert got["bwt_r"].tolist() == [1, 1, 0, 2, 0]


@pytest.mark.parametrize("rate", RATES)
def test_oracle_idx_round_trip_keeps_the_rate(tmp_path, rate):
    case_id = f"rate{rate}-s6"
    idx = oracle_index(case_id)
    p1, p2 = tmp_path / "a.idx", tmp_path / "b.idx"
    idx.write(p1)
    raw = p1.read_bytes()
    at = rate_offset(6, len(records(case_id)))
    assert int.from_bytes(raw[at:at + 8], "little") == rate
    back = O.Index.read(p1)
    back.write(p2)
    assert p2.read_bytes() == raw
    # the rate bounds the LF walk of every locate: same hits and same walk lengths
    recs = list(records(case_id))
    pats = np.stack([recs[0][j:j + 20] for j in range(5, 2900, 97)])
    sch = O.scheme("h2-k2", 0, 1, 20)
    h1, c1 = idx.search(pats, sch)
    h2, c2 = back.search(pats, sch)
    assert np.array_equal(hits_as_rows(h1), hits_as_rows(h2)) and len(h1) >= len(pats)
    assert c1 == c2 and (c1["lf_steps"] == 0) == (rate == 1)


def test_lf_steps_tell_the_rates_apart():
    """What lets the GPU tests' counter comparison catch a wrong walk bound or
    sample index: over the same text and patterns the oracle takes no LF step
    at rate 1 (every row is sampled) and more with every rate of the table,
    for the same rows."""
    runs = [locate_inputs(c.id) for c in LOCATE_CASES if c.kind == "rate" and c.sigma == 6]
    steps = [cnt["lf_steps"] for _, _, cnt in runs]
    print("lf_steps at rates", RATES, steps)
    assert steps[0] == 0 and all(a < b for a, b in zip(steps, steps[1:])), steps
    assert all(np.array_equal(rows, runs[0][1]) for _, rows, _ in runs) and len(runs[0][1]) >= 100


def test_locate_cases_have_hits():
    for c in LOCATE_CASES:
        pats, rows, cnt = locate_inputs(c.id)
        assert len(pats) == 100 and len(np.unique(rows[:, 0])) >= 90 and cnt["rows"] == len(rows), c.id


@pytest.mark.parametrize("bad", [0, 1 << 32])
def test_library_refuses_an_impossible_rate_before_any_device_call(tmp_path, bad):
    """parseIdx runs before the context is made, so the refusal of a rate of 0
    or one past 32 bits needs no GPU: the message is the parser's, not that of
    a missing device."""
    import sahara_amd as sa
    case_id = "n64-split"
    oracle_index(case_id).write(tmp_path / "o.idx")
    image = bytearray((tmp_path / "o.idx").read_bytes())
    at = rate_offset(6, len(records(case_id)))
    assert int.from_bytes(image[at:at + 8], "little") == 16
    image[at:at + 8] = bad.to_bytes(8, "little")
    with pytest.raises(sa.SaharaError, match="sampling rate"):
        sa.BiFMIndex.from_bytes(bytes(image))


@pytest.mark.parametrize("rate", [16, 3])
@pytest.mark.parametrize("sigma,edit,m,k", DEGENERATE)
def test_degenerate_texts_oracle_equals_bruteforce(sigma, edit, m, k, rate):
    recs, pats = degenerate(sigma, edit, m, k)
    sch = O.scheme("h2-k2", 0, k, m, hamming=not edit)
    rows = hits_as_rows(O.Index.build(list(recs), sigma, rate).search(pats, sch, edit=edit)[0])
    assert pset(rows) == pset(hits_as_rows(O.bruteforce(list(recs), pats, k, edit=edit)))
    # exactly the records that can hold an occurrence do (m - k symbols with k insertions, m without
    # indels): more than half of them in the edit sets with k > 0
    can = [i for i, r in enumerate(recs) if len(r) >= m - (k if edit else 0)]
    assert np.unique(rows[:, 1]).tolist() == can
    assert not (edit and k) or len(can) > len(recs) // 2


@pytest.mark.parametrize("rate", [16, 3])
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_texts_oracle_equals_bruteforce(name, rate):
    recs, m, k, pats = tiny(name)
    rows = hits_as_rows(O.Index.build(recs, 6, rate).search(pats, O.scheme("h2-k2", 0, k, m))[0])
    assert pset(rows) == pset(hits_as_rows(O.bruteforce(recs, pats, k)))
    if name == "acg-c-m4":
        first = rows[rows[:, 0] == 0]
        assert first[:, 1:].tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 2], [0, 0, 2], [0, 0, 2], [0, 1, 2]]
    else:
        assert len(rows) == 0
