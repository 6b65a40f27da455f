"""The host decoder of compact hit records (csrc/compact_hit.h), which the
library's expander and the command line's writers share:
tests/compact_hit_check.cpp, built alone under the address and
undefined-behaviour sanitizers (CPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_hit(tmp_path):
    exe = tmp_path / "compact_hit_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "compact_hit_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
