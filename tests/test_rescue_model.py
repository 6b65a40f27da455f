"""tests/rescue_model.py, the checker of the mate rescue, on the planted case
of tests/rescue_case.py: the consequences docs/semantics.md "Mate rescue"
states, hand-written rows, and the scan's brute force against the alignment
model start by start (CPU)."""
import numpy as np
import pytest

from align_model import align, concat_text
from pairs_case import K, M
from pairs_model import pairs
from rescue_case import CAP, KS, MAIN, SETTINGS, check, expect, model
from rescue_model import anchors, rescue, scan, window


def as_set(rows):
    return set(map(tuple, np.asarray(rows, np.uint64).reshape(-1, 4).tolist()))


def test_the_planted_case_holds():
    check()


def test_a_bound_at_the_searchs_own_adds_no_row():
    c = check()
    for s in SETTINGS:
        got, st = model(s, K)
        assert np.array_equal(got, c["want"]) and st["rescued"] == 0 and st["anchors"] > 0, s


@pytest.mark.parametrize("Kr", KS)
def test_added_rows_lie_above_the_searchs_bound_and_pair_with_their_anchor(Kr):
    c = check()
    have = as_set(c["want"])
    for s in SETTINGS:
        got, st = model(s, Kr)
        new = as_set(got) - have
        assert len(new) == st["rescued"] == len(got) - len(c["want"]) and new, s
        assert all(K < r[3] <= Kr for r in new), s
        kept = as_set(pairs(got, M, *s))
        assert new <= kept  # every rescued record is kept, beside the anchor that found it
        idx, _ = anchors(c["want"], c["recs"], M, *s, 0)
        dmin, dmax = max(s[0], M) - M, s[1] - M
        for q, rec, pos, _ in new:
            mine = [tuple(r) for r in c["want"][idx].tolist() if r[0] == q ^ 3 and r[1] == rec]
            near = [r for r in mine if (lambda w: w and w[0] <= pos <= w[1])(window(r[0], r[2], dmin, dmax, len(c["recs"][rec])))]
            assert near and all(r in kept for r in near), (s, q, pos)
        # with the pair rule applied, a superset of the pairs-only rows
        assert as_set(pairs(c["want"], M, *s)) <= kept and np.array_equal(pairs(got, M, *s), expect(s, Kr))


def test_the_cap_takes_whole_queries():
    c = check()
    for Kr in KS:
        full, capped = model(MAIN, Kr), model(MAIN, Kr, CAP)
        assert capped[1]["capped_queries"] == 1 and capped[1]["anchors"] < full[1]["anchors"]
        assert as_set(capped[0]) < as_set(full[0])
        assert model(MAIN, Kr, 32)[1] == full[1]


HANDFUL = ("errors", "at hi", "clipped at end", "clipped at 0", "tie across rounds", "cheaper later", "N in both")


def test_the_scan_equals_the_alignment_model_start_by_start():
    """e* of "Alignments" at every start of the window, the least taken with
    ties to the smaller start, for a handful of anchors."""
    c = check()
    T = concat_text(c["recs"])
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in c["recs"]])])
    w = c["want"]
    idx, _ = anchors(w, c["recs"], M, *MAIN, 0)
    picked = {}
    for e in c["plan"]:
        if e["kind"] in HANDFUL and e["kind"] not in picked:
            picked[e["kind"]] = (4 * e["pair"] + e["anchor"][0], e["seq"], e["anchor"][1])
    assert len(picked) == len(HANDFUL)
    dmin, dmax = MAIN[0] - M, MAIN[1] - M
    for kind, (q, s, p) in picked.items():
        assert (q, s, p) in set(map(tuple, w[idx][:, :3].tolist())), kind
        lo, hi = window(q, p, dmin, dmax, len(c["recs"][s]))
        pat = c["pats"][q ^ 3]
        for Kr, edit in ((3, True), (8, True), (8, False)):
            best = None
            for at in range(lo, hi + 1):
                res = align(pat, T, int(starts[s]) + at, Kr, edit=edit)
                if res is not None and (best is None or res[0] < best[0]):
                    best = (res[0], at)
            assert scan(c["recs"][s], pat, lo, hi, Kr, edit) == best, (kind, Kr, edit)


def test_rows_written_by_hand():
    rng = np.random.default_rng(3)
    rec = np.array([1, 2, 3, 5], np.uint8)[rng.integers(0, 4, size=400)]
    m = 20
    a, b = 30, 130
    mate = rec[b:b + m].copy()
    for j in (3, 9, 15):
        mate[j] = 1 + mate[j] % 3 if mate[j] != 5 else 1
    pats = np.zeros((4, m), np.uint8)
    pats[0], pats[3] = rec[a:a + m], mate
    pats[1], pats[2] = 5, 5  # (never looked at: no anchor has them as partner)
    rows = np.array([[0, 0, a, 0], [0, 0, a, 2]], np.uint64)
    st = {}
    got = rescue(rows, pats, [rec], m, 40, 140, 3, True, 0, st)
    assert np.array_equal(got, np.array([[0, 0, a, 0], [0, 0, a, 2], [3, 0, b, 3]], np.uint64))
    assert st == dict(anchors=1, capped_queries=0, starts=101, rescued=1)  # the duplicate is no anchor of its own
    assert np.array_equal(rescue(rows, pats, [rec], m, 40, 140, 2), rows)
    assert np.array_equal(rescue(rows, pats, [rec], m, 40, 119, 3), rows)  # the mate one start past the window
    assert len(rescue(rows, pats, [rec], m, 40, 120, 3)) == 3
    with pytest.raises(ValueError):
        rescue(rows, pats, [rec], m, 0, m + 4096, 3)
    with pytest.raises(ValueError):
        rescue(rows, pats, [rec], m, 40, 140, 9)
