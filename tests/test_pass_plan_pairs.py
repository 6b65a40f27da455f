"""Batch boundaries and query shards in whole pairs (csrc/pass_plan.h and
cli/shard.h with a granularity): tests/pass_plan_pairs_check.cpp, built alone
under the address and undefined-behaviour sanitizers (CPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batches_and_shards_hold_whole_pairs(tmp_path):
    exe = tmp_path / "pass_plan_pairs_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "pass_plan_pairs_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
