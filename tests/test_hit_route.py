"""Where a call's hits go (csrc/hit_route.h): the call's route and the
decision for one batch against hand-written values, a restatement of the
earlier flag logic and the invariants between sort and copy, built alone under
the address and undefined-behaviour sanitizers (CPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hit_route_decisions(tmp_path):
    exe = tmp_path / "hit_route_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "hit_route_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
