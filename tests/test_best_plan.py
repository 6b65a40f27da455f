"""The geometry rule of a pass of several rounds (besthits) against
hand-derived values, built alone under the address and undefined-behaviour
sanitizers (CPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rounds_plan_arithmetic(tmp_path):
    exe = tmp_path / "pass_plan_rounds_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "pass_plan_rounds_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
