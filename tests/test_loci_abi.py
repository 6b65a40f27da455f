"""The loci calls at the C ABI: exported, declared, mirrored, refusing NULL
arguments with a message, the stats record's size (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import sahara_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_set_loci", "sahara_gpu_loci_stats"]


def test_symbols_exported_declared_and_mirrored():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(void\* ctx," % name, text), name
        assert name in sa.EXPORTED
    assert callable(sa.BiFMIndex.set_loci) and callable(sa.BiFMIndex.loci_stats)


def test_null_arguments_are_refused_with_a_message():
    L = sa.lib()
    s = sa.LociStats(1, 2, 3, 4.0)
    assert L.sahara_gpu_set_loci(None, 1, 2) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_loci_stats(None, C.byref(s)) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert (s.hits_in, s.loci, s.batches, s.kernel_ms) == (1, 2, 3, 4.0)  # untouched
    assert L.sahara_gpu_loci_stats(None, None) < 0
    assert b"null output" in L.sahara_gpu_last_error()


def test_stats_record_is_32_bytes(tmp_path):
    assert C.sizeof(sa.LociStats) == 32
    assert [n for n, _ in sa.LociStats._fields_] == ["hits_in", "loci", "batches", "kernel_ms"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   'static_assert(sizeof(sahara_loci_stats) == 32, "size");\n'
                   'static_assert(offsetof(sahara_loci_stats, hits_in) == 0, "hits_in");\n'
                   'static_assert(offsetof(sahara_loci_stats, loci) == 8, "loci");\n'
                   'static_assert(offsetof(sahara_loci_stats, batches) == 16, "batches");\n'
                   'static_assert(offsetof(sahara_loci_stats, kernel_ms) == 24, "kernel_ms");\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
