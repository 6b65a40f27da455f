"""The text kernel's micro-step itself (csrc/text_step.h: textStep, the code a
lane runs) on a CPU: tests/text_step_check.cpp runs it as a DFS over the cases
of tests/test_text_model.py and holds it to the plain P0 DFS's leaves and, step
for step, to the model's node count — built alone under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from text_model import chain, chain_cases, plain, true_read_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_cases(path):
    """Groups 1-5: the seeds of test_chain_step_equals_plain_dfs; group 6: the
    m = 100, k = 2, depth-16 tasks of test_pruning_on_true_reads. Per case one
    search's pi, l, u, then P, T and the tasks; per task the leaf multiset of
    plain() and the nodes chain() processes at RUN = 32, CHAIN = 25."""
    groups = [(seed, 100, chain_cases(seed)) for seed in (1, 2, 3, 4, 5)] + [(6, 0, true_read_cases())]
    lines = []
    for group, need, cases in groups:  # a group must check more than `need` tasks
        for P, T, sch, edit, cap, tasks in cases:
            pi, l, u, _ = sch
            lines.append("case %d %d %d %d %d %d %d" % (group, need, len(pi), len(T), int(edit), cap, len(tasks)))
            for row in (pi, l, u, P, T):
                lines.append(" ".join(str(int(v)) for v in row))
            for task in tasks:
                stats = {}
                leaves = plain(P, T, task, sch, edit)
                assert chain(P, T, task, sch, edit, cap=cap, stats=stats) == leaves
                lines.append(" ".join(str(v) for v in task + (stats["steps"], len(leaves))))
                lines.append(" ".join("%d %d %d" % (xs, e, n) for (xs, e), n in sorted(leaves.items())))
    lines.append("end")
    path.write_text("\n".join(lines) + "\n")


def test_text_step_on_host(tmp_path):
    exe = tmp_path / "text_step_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "text_step_check.cpp"), "-o", str(exe)], check=True)
    cases = tmp_path / "cases.txt"
    write_cases(cases)
    p = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
