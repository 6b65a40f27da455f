"""The mate-rescue calls at the C ABI: exported, declared, mirrored, refusing
NULL arguments and a bound outside [1, 8] with a message, the stats record's
size and that the records beside it kept theirs (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sahara_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_set_rescue", "sahara_gpu_rescue_stats"]


def test_symbols_exported_declared_and_mirrored():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(void\* ctx," % name, text), name
        assert name in sa.EXPORTED
    assert callable(sa.BiFMIndex.set_rescue) and callable(sa.BiFMIndex.rescue_stats)
    assert re.search(r"#define\s+SAHARA_RESCUE_MAX_WINDOW\s+4096\b", text)


def test_the_setter_refuses_a_null_context_and_a_bound_outside_1_to_8():
    L = sa.lib()
    s = sa.RescueStats(1, 2, 3, 4, 5, 6.0)
    assert L.sahara_gpu_set_rescue(None, 1, 3, 64) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    for bad in (0, 9, 0xFFFFFFFF):
        assert L.sahara_gpu_set_rescue(None, 1, bad, 64) < 0  # (the arguments are looked at before the context)
        assert b"max_err must be in [1, 8]" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_set_rescue(None, 0, 9, 0) < 0  # turning it off takes any values
    assert b"null context" in L.sahara_gpu_last_error()
    assert L.sahara_gpu_rescue_stats(None, C.byref(s)) < 0
    assert b"null context" in L.sahara_gpu_last_error()
    assert (s.anchors, s.capped_queries, s.starts, s.rescued, s.batches, s.kernel_ms) == (1, 2, 3, 4, 5, 6.0)  # untouched
    assert L.sahara_gpu_rescue_stats(None, None) < 0
    assert b"null output" in L.sahara_gpu_last_error()


def test_stats_record_is_48_bytes_and_the_others_keep_their_sizes(tmp_path):
    assert C.sizeof(sa.RescueStats) == 48
    assert [n for n, _ in sa.RescueStats._fields_] == ["anchors", "capped_queries", "starts", "rescued", "batches",
                                                       "kernel_ms"]
    assert C.sizeof(sa.PairsStats) == 40 and C.sizeof(sa.LociStats) == 32
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   'static_assert(sizeof(sahara_rescue_stats) == 48, "size");\n'
                   'static_assert(offsetof(sahara_rescue_stats, anchors) == 0, "anchors");\n'
                   'static_assert(offsetof(sahara_rescue_stats, capped_queries) == 8, "capped_queries");\n'
                   'static_assert(offsetof(sahara_rescue_stats, starts) == 16, "starts");\n'
                   'static_assert(offsetof(sahara_rescue_stats, rescued) == 24, "rescued");\n'
                   'static_assert(offsetof(sahara_rescue_stats, batches) == 32, "batches");\n'
                   'static_assert(offsetof(sahara_rescue_stats, kernel_ms) == 40, "kernel_ms");\n'
                   'static_assert(sizeof(sahara_pairs_stats) == 40 && sizeof(sahara_loci_stats) == 32, "neighbours");\n'
                   'static_assert(sizeof(sahara_hit) == 24 && sizeof(sahara_alignment) == 24, "records");\n'
                   'static_assert(SAHARA_RESCUE_MAX_WINDOW == 4096 && SAHARA_ALIGN_MAX_ERR == 8, "limits");\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_refuses_bad_settings_before_the_library():
    class Handle(sa.BiFMIndex):
        def __init__(self):  # no index: the checks below never reach the library
            self._h = None
    for bad in ((-1, 64), (3, -1), (1 << 32, 0), (3, 1 << 32)):
        with pytest.raises(ValueError):
            Handle.set_rescue(Handle(), *bad)
