"""The pair calls at the C ABI: exported, declared, mirrored, refusing NULL
arguments with a message, the stats record's size; and the argument errors of
`sahara search --paired` that end before the index is asked (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import sahara_amd as sa
from test_cli import run, write
from test_golden import GOLD, IDX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_set_pairs", "sahara_gpu_pairs_stats"]


def test_symbols_exported_declared_and_mirrored():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(void\* ctx," % name, text), name
        assert name in sa.EXPORTED
    assert callable(sa.BiFMIndex.set_pairs) and callable(sa.BiFMIndex.pairs_stats)


def test_null_arguments_are_refused_with_a_message():
    L = sa.lib()
    s = sa.PairsStats(1, 2, 3, 4, 5.0)
    assert L.sahara_gpu_set_pairs(None, 1, 100, 300) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_set_pairs(None, 1, 300, 100) < 0  # (the arguments are looked at before the context)
    assert b"min_fragment is above max_fragment" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_set_pairs(None, 0, 300, 100) < 0  # turning it off takes any values
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_pairs_stats(None, C.byref(s)) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert (s.hits_in, s.kept, s.pairs, s.batches, s.kernel_ms) == (1, 2, 3, 4, 5.0)  # untouched
    assert L.sahara_gpu_pairs_stats(None, None) < 0
    assert b"null output" in L.sahara_gpu_last_error()


def test_stats_record_is_40_bytes(tmp_path):
    assert C.sizeof(sa.PairsStats) == 40
    assert [n for n, _ in sa.PairsStats._fields_] == ["hits_in", "kept", "pairs", "batches", "kernel_ms"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   'static_assert(sizeof(sahara_pairs_stats) == 40, "size");\n'
                   'static_assert(offsetof(sahara_pairs_stats, hits_in) == 0, "hits_in");\n'
                   'static_assert(offsetof(sahara_pairs_stats, kept) == 8, "kept");\n'
                   'static_assert(offsetof(sahara_pairs_stats, pairs) == 16, "pairs");\n'
                   'static_assert(offsetof(sahara_pairs_stats, batches) == 24, "batches");\n'
                   'static_assert(offsetof(sahara_pairs_stats, kernel_ms) == 32, "kernel_ms");\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_refuses_bad_settings_before_the_library():
    class Handle(sa.BiFMIndex):
        def __init__(self):  # no index: the checks below never reach the library
            self._h = None
    import pytest
    for bad in ((-1, 10), (0, 1 << 32), (5, None)):
        with pytest.raises(ValueError):
            Handle.set_pairs(Handle(), *bad)


def test_cli_argument_errors(tmp_path):
    base = ["search", "-i", os.path.join(GOLD, IDX["a"])]
    reads = os.path.join(GOLD, "reads_a.fa")
    rc, _, err = run(*base, "-q", reads, "--paired", "--no-reverse")
    assert rc == 1 and "--paired" in err and "--no-reverse" in err
    rc, _, err = run(*base, "-q", reads, "--paired", "--limit_queries", 6)
    assert rc == 1 and "--limit_queries must be a multiple of 4" in err
    rc, _, err = run(*base, "-q", reads, "--paired", "--min-fragment", 300, "--max-fragment", 200)
    assert rc == 1 and "--min-fragment is above --max-fragment" in err
    rc, _, err = run(*base, "-q", reads, "--max-fragment", 200)
    assert rc == 1 and "need --paired" in err
    odd = write(tmp_path / "odd.fa", ">a\nACGTACGTAC\n>b\nACGTACGTAA\n>c\nACGTACGTTT\n")
    rc, _, err = run(*base, "-q", odd, "--paired")
    assert rc == 1 and "3 reads, an odd number" in err
    even = write(tmp_path / "even.fa", ">a\nACGTACGTAC\n>b\nACGTACGTAA\n")
    rc, _, err = run(*base, "-q", even, "--paired", "--max-fragment", 9)
    assert rc == 1 and "--max-fragment 9 is below the read length 10" in err
