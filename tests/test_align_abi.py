"""The alignment calls at the C ABI: exported, declared, mirrored, the record's
layout on both sides, a NULL context refused, and sahara_cigar (host only) on
hand-made records. No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import align_model as am
import sahara_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_align", "sahara_gpu_align_packed_compact", "sahara_cigar"]


def test_symbols_exported_declared_and_mirrored():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(" % name, text), name
        assert name in sa.EXPORTED
    for name in ("ALIGN_DTYPE", "align", "align_packed_compact", "cigar"):
        assert hasattr(sa, name) and name in sa.__all__, name


def test_record_is_24_bytes_on_both_sides(tmp_path):
    assert sa.ALIGN_DTYPE.itemsize == 24
    assert [sa.ALIGN_DTYPE.fields[f][1] for f in ("err", "ref_len", "edit")] == [0, 4, 8]
    assert sa.ALIGN_MAX_ERR == am.MAX_ERR == 8 and sa.ALIGN_NONE == am.NONE == 0xFFFFFFFF
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   "static_assert(sizeof(sahara_alignment) == 24, \"size\");\n"
                   "static_assert(offsetof(sahara_alignment, err) == 0, \"err\");\n"
                   "static_assert(offsetof(sahara_alignment, ref_len) == 4, \"ref_len\");\n"
                   "static_assert(offsetof(sahara_alignment, edit) == 8, \"edit\");\n"
                   "static_assert(SAHARA_ALIGN_MAX_ERR == 8 && SAHARA_ALIGN_NONE == 0xFFFFFFFFu, \"constants\");\n"
                   "static_assert(sizeof(sahara_stats) == 344, \"sahara_stats is left alone\");\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_an_error():
    L = sa.lib()
    ranks = (C.c_uint8 * 4)(1, 2, 3, 1)
    hits = np.zeros(1, sa.HIT_DTYPE)
    out = np.full(1, 7, sa.ALIGN_DTYPE)
    blocks = sa.HitBlocks()
    calls = {
        NEW[0]: lambda: L.sahara_gpu_align(None, ranks, 1, 4, 1, 2, hits.ctypes.data_as(C.c_void_p), 1,
                                           out.ctypes.data_as(C.c_void_p)),
        NEW[1]: lambda: L.sahara_gpu_align_packed_compact(None, ranks, 0, None, 0, 1, 4, 1, 0, 1, 2, C.byref(blocks),
                                                          out.ctypes.data_as(C.c_void_p)),
    }
    for name, call in calls.items():
        assert call() < 0, name
        assert b"null context" in L.sahara_gpu_last_error(), name
    assert out["err"][0] == 7 and out["ref_len"][0] == 7  # untouched


def rec(err, ref_len, edits):
    r = np.zeros(1, sa.ALIGN_DTYPE)
    r["err"], r["ref_len"] = err, ref_len
    for s, (qpos, kind) in enumerate(edits):
        r["edit"][0, s] = (qpos << 2) | kind
    return r[0]


def test_cigar_of_hand_made_records():
    X, I, D = am.KIND_X, am.KIND_I, am.KIND_D
    cases = [
        (100, [], "100="),                                  # no edits
        (100, [(57, X)], "57=1X42="),
        (100, [(0, X)], "1X99="),
        (100, [(99, X)], "99=1X"),
        (9, [(3, D)], "3=1D6="),
        (10, [(4, I)], "4=1I5="),
        (10, [(9, I)], "9=1I"),                             # an I may be last
        (20, [(5, D), (5, X)], "5=1D1X14="),                # two edits at one qpos
        (20, [(5, D), (5, D)], "5=2D15="),                  # runs
        (20, [(3, X), (4, X), (5, X)], "3=3X14="),
        (20, [(7, I), (8, I), (12, X)], "7=2I3=1X7="),
        (16383, [(16382, X)], "16382=1X"),
        (12, [(0, X), (1, I), (3, D), (5, X), (6, X), (8, I), (9, I), (11, X)], "1X1I1=1D2=2X1=2I1=1X"),
    ]
    for m, edits, want in cases:
        n_i = sum(k == I for _, k in edits)
        n_d = sum(k == D for _, k in edits)
        assert sa.cigar(rec(len(edits), m - n_i + n_d, edits), m) == want, (m, edits)
        assert am.cigar(edits, m) == want, (m, edits)
    assert sa.cigar(rec(sa.ALIGN_NONE, 0, []), 100) is None  # a NONE record


def test_cigar_buffer_too_small():
    L = sa.lib()
    r = np.zeros(1, sa.ALIGN_DTYPE)
    r["err"], r["ref_len"] = 1, 100
    r["edit"][0, 0] = (57 << 2) | am.KIND_X
    want = b"57=1X42="
    for cap in range(0, 12):
        buf = C.create_string_buffer(b"#" * 16, 16)
        n = L.sahara_cigar(r.ctypes.data_as(C.c_void_p), 100, buf, cap)
        if cap >= len(want) + 1:  # the text and its terminator
            assert n == len(want) and buf.raw[:n + 1] == want + b"\0"
        else:
            assert n == -1
        assert buf.raw[max(cap, 0):] == b"#" * (16 - cap)  # nothing written past cap
