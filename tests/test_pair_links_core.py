"""The pure functions of the pair stage's links (csrc/pair_links_core.h):
tests/pair_links_core_check.cpp, built alone under the address and
undefined-behaviour sanitizers (CPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_links_core(tmp_path):
    exe = tmp_path / "pair_links_core_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "pair_links_core_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
