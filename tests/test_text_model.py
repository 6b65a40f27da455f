"""The text kernel's chain micro-step (modelled in tests/text_model.py) yields
the same leaf multiset as the plain P0 DFS against the text, from arbitrary
DFS states, within the 2k + 2 stack bound."""
import pytest

from text_model import chain, chain_cases, plain, true_read_cases


@pytest.mark.parametrize("run,chain_len", [(16, 8), (32, 16), (32, 25)])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_chain_step_equals_plain_dfs(seed, run, chain_len):
    checked = 0
    for P, T, sch, edit, cap, tasks in chain_cases(seed):
        for task in tasks:
            assert chain(P, T, task, sch, edit, cap=cap, RUN=run, CHAIN=chain_len) == plain(P, T, task, sch, edit)
            checked += 1
    assert checked > 100


def test_pruning_on_true_reads():
    """h2-k2, m = 100, k = 2: reads with two random edits against their text.
    From every task the FM phase could hand over at depth 16, the pruned step
    (nodes two errors below their bound keep only viable error children) gives
    the plain DFS's leaves, in fewer micro-steps."""
    steps = {True: {}, False: {}}
    for P, T, sch, edit, cap, tasks in true_read_cases():
        for task in tasks:
            want = plain(P, T, task, sch, edit)
            for prune in (True, False):
                assert chain(P, T, task, sch, edit, cap=cap, PRUNE=prune, stats=steps[prune]) == want
    assert steps[True]["steps"] < 0.85 * steps[False]["steps"]
