"""The besthits twins of the reads calls at the C ABI: exported, declared,
refusing a NULL context, and the two stats fields taken out of `reserved`
without moving anything (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import sahara_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sahara_hip.h")
NEW = ["sahara_gpu_search_best_reads", "sahara_gpu_search_best_packed", "sahara_gpu_search_best_packed_compact"]

# sahara_stats before the two fields were named: 344 bytes, reserved[8] at byte 280
STATS_BYTES, RESERVED_AT = 344, 280


def test_symbols_exported_and_declared():
    L = sa.lib()
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\(void\* ctx," % name, text), name
        assert name in sa.EXPORTED


def test_null_context_is_an_error():
    L = sa.lib()
    n = C.c_uint64()
    out = C.c_void_p()
    blocks = sa.HitBlocks()
    ns = (C.c_uint32 * 1)(1)
    z = (C.c_uint32 * 4)()
    codes = (C.c_uint8 * 4)()
    calls = {
        NEW[0]: lambda: L.sahara_gpu_search_best_reads(None, codes, 1, 4, 1, 0, z, z, z, ns, 1, 0, C.byref(out),
                                                       C.byref(n)),
        NEW[1]: lambda: L.sahara_gpu_search_best_packed(None, codes, 0, None, 0, 1, 4, 1, 0, z, z, z, ns, 1, 0,
                                                        C.byref(out), C.byref(n)),
        NEW[2]: lambda: L.sahara_gpu_search_best_packed_compact(None, codes, 0, None, 0, 1, 4, 1, 0, z, z, z, ns, 1,
                                                                C.byref(blocks)),
    }
    for name, call in calls.items():
        assert call() < 0, name
        assert b"null context" in L.sahara_gpu_last_error(), name
    assert not out.value and blocks.n_hits == 0 and not blocks.recs


def test_stats_fields_sit_in_the_former_reserved_area(tmp_path):
    S = sa.Stats
    assert C.sizeof(S) == STATS_BYTES
    assert S.best_rounds.offset == RESERVED_AT and S.best_skipped.offset == RESERVED_AT + 8
    assert S.reserved.offset == RESERVED_AT + 16 and S.reserved.size == STATS_BYTES - RESERVED_AT - 16
    assert {"best_rounds", "best_skipped"} <= set(S().as_dict())
    # ... and the C struct says the same
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "sahara_hip.h"\n'
                   "static_assert(sizeof(sahara_stats) == %d, \"size\");\n"
                   "static_assert(offsetof(sahara_stats, best_rounds) == %d, \"best_rounds\");\n"
                   "static_assert(offsetof(sahara_stats, best_skipped) == %d, \"best_skipped\");\n"
                   "static_assert(offsetof(sahara_stats, reserved) == %d, \"reserved\");\n"
                   % (STATS_BYTES, RESERVED_AT, RESERVED_AT + 8, RESERVED_AT + 16))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
