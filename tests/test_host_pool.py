"""The context's host thread pools and the pass's issuer / finisher handshake
under the thread and address sanitizers, and the HIP-free part of a pass's
plan against hand-derived values (CPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_host_pools_are_clean_under_sanitizers(tmp_path, sanitize):
    exe = tmp_path / "host_pool_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitize,
                    os.path.join(ROOT, "tests", "host_pool_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])


def test_pass_plan_arithmetic(tmp_path):
    exe = tmp_path / "pass_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "pass_plan_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
