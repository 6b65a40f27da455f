// Symbols as three bit planes, as the text kernel's LDS holds the window and
// the pattern, for the host checks of the step headers (text_step_check.cpp,
// fm_step_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../sahara_amd/csrc/text_step.h"

// n symbols as three bit planes, 32 symbols per word
struct Packed {
    std::vector<uint32_t> b[3];
    long n = 0;
    explicit Packed(const std::vector<uint32_t>& s) : n((long)s.size()) {
        for (auto& w : b) w.assign((s.size() + 31) / 32, 0u);
        for (size_t i = 0; i < s.size(); ++i)
            for (int p = 0; p < 3; ++p) b[p][i / 32] |= ((s[i] >> p) & 1u) << (i % 32);
    }
    uint32_t at(long i) const {
        const size_t w = (size_t)i / 32, o = (size_t)i % 32;
        return ((b[0][w] >> o) & 1u) | (((b[1][w] >> o) & 1u) << 1) | (((b[2][w] >> o) & 1u) << 2);
    }
    // 32 symbols in chain order from offset o; junk(q) stands outside the array
    template <class Junk>
    sahara::Planes chain(uint32_t o, bool fwd, Junk junk) const {
        sahara::Planes r = {0u, 0u, 0u};
        for (long j = 0; j < 32; ++j) {
            const long q = fwd ? (long)o + j : (long)o - 1 - j;
            const uint32_t s = q >= 0 && q < n ? at(q) : junk(q);
            r.b0 |= (s & 1u) << j;
            r.b1 |= ((s >> 1) & 1u) << j;
            r.b2 |= ((s >> 2) & 1u) << j;
        }
        return r;
    }
};
