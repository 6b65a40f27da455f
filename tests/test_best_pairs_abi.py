"""The best-pairs calls at the C ABI: exported, declared, mirrored, refusing
NULL arguments with a message, the records' sizes; and the argument errors of
`sahara search --best-pairs` that end before the index is asked (no GPU
needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sahara_amd as sa
from test_cli import run
from test_golden import GOLD, IDX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_set_best_pairs", "sahara_gpu_pair_summary", "sahara_gpu_best_pairs_stats"]


def test_symbols_exported_declared_and_mirrored():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(void\* ctx," % name, text), name
        assert name in sa.EXPORTED
    for method in ("set_best_pairs", "best_pairs_stats", "pair_summary"):
        assert callable(getattr(sa.BiFMIndex, method))
    assert "PAIR_SUMMARY_DTYPE" in sa.__all__ and "PAIR_NONE" in sa.__all__ and sa.PAIR_NONE == 255


def test_null_arguments_are_refused_with_a_message():
    L = sa.lib()
    s = sa.BestPairsStats(1, 2, 3, 4, 5, 6.0)
    assert L.sahara_gpu_set_best_pairs(None, 1, 0) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_set_best_pairs(None, 1, 31) < 0  # (the arguments are looked at before the context)
    assert b"delta must be in [0, 30]" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_set_best_pairs(None, 0, 31) < 0  # turning it off takes any value
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_best_pairs_stats(None, C.byref(s)) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert (s.hits_in, s.kept, s.pairs, s.unique_pairs, s.batches, s.kernel_ms) == (1, 2, 3, 4, 5, 6.0)  # untouched
    assert L.sahara_gpu_best_pairs_stats(None, None) < 0
    assert b"null output" in L.sahara_gpu_last_error()
    n = C.c_uint64(7)
    assert L.sahara_gpu_pair_summary(None, None, 0, C.byref(n)) < 0
    assert b"null context" in L.sahara_gpu_last_error() and n.value == 7


def test_records_are_8_and_48_bytes(tmp_path):
    assert C.sizeof(sa.BestPairsStats) == 48 and sa.PAIR_SUMMARY_DTYPE.itemsize == 8
    assert [n for n, _ in sa.BestPairsStats._fields_] == ["hits_in", "kept", "pairs", "unique_pairs", "batches",
                                                          "kernel_ms"]
    assert [(n, sa.PAIR_SUMMARY_DTYPE.fields[n][1]) for n in sa.PAIR_SUMMARY_DTYPE.names] == \
        [("best", 0), ("next", 1), ("n_fwd", 2), ("n_rev", 4), ("reserved", 6)]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   'static_assert(sizeof(sahara_pair_summary) == 8, "size");\n'
                   'static_assert(offsetof(sahara_pair_summary, best) == 0, "best");\n'
                   'static_assert(offsetof(sahara_pair_summary, next) == 1, "next");\n'
                   'static_assert(offsetof(sahara_pair_summary, n_fwd) == 2, "n_fwd");\n'
                   'static_assert(offsetof(sahara_pair_summary, n_rev) == 4, "n_rev");\n'
                   'static_assert(offsetof(sahara_pair_summary, reserved) == 6, "reserved");\n'
                   'static_assert(sizeof(sahara_best_pairs_stats) == 48, "size");\n'
                   'static_assert(offsetof(sahara_best_pairs_stats, unique_pairs) == 24, "unique_pairs");\n'
                   'static_assert(offsetof(sahara_best_pairs_stats, kernel_ms) == 40, "kernel_ms");\n'
                   'static_assert(sizeof(sahara_pairs_stats) == 40, "the pair stage\'s record stands");\n'
                   'static_assert(SAHARA_BEST_PAIRS_MAX_DELTA == 30, "delta");\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_refuses_bad_settings_before_the_library():
    class Handle(sa.BiFMIndex):
        def __init__(self):  # no index: the checks below never reach the library
            self._h = None
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            Handle.set_best_pairs(Handle(), bad)


def test_cli_argument_errors_and_help():
    base = ["search", "-i", os.path.join(GOLD, IDX["a"]), "-q", os.path.join(GOLD, "reads_a.fa")]
    rc, _, err = run(*base, "--best-pairs")
    assert rc == 1 and "--best-pairs needs --paired" in err
    for flag in (("--pair-delta", 1), ("--pair-summary", "x.tsv")):
        rc, _, err = run(*base, "--paired", *flag)
        assert rc == 1 and "need --best-pairs" in err, flag
    rc, _, err = run(*base, "--paired", "--best-pairs", "--pair-delta", 31)
    assert rc == 1 and "--pair-delta is at most 30" in err
    rc, out, _ = run("--help")
    assert rc == 0 and all(x in out for x in ("--best-pairs", "--pair-delta <d>", "--pair-summary <file>"))
