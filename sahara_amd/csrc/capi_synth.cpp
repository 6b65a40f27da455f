// capi_synth.cpp — the host-only helpers of the C ABI (include/sahara_hip.h):
// synthetic references and reads, the 2-bit packer, the reverse-complement
// interleave, CIGAR strings.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ctx.h"
#include "idx_format.h"

using namespace sahara;

extern "C" {

int sahara_synth_reference(uint64_t seed, uint32_t sigma, const uint64_t* rec_lens, uint64_t n_records,
                           uint8_t* out) {
    return guarded([&] {
        if (sigma != 5 && sigma != 6) throw Error("sigma must be 5 or 6");
        const uint8_t code[4] = {1, 2, 3, (uint8_t)(sigma == 6 ? 5 : 4)};
        uint64_t total = 0;
        for (uint64_t r = 0; r < n_records; ++r) total += rec_lens[r];
        std::mt19937_64 gen(seed);
        uint64_t i = 0;
        for (; i + 32 <= total; i += 32) {
            uint64_t x = gen();
            for (int j = 0; j < 32; ++j) out[i + j] = code[(x >> (2 * j)) & 3u];
        }
        if (i < total) {
            uint64_t x = gen();
            for (int j = 0; i < total; ++i, ++j) out[i] = code[(x >> (2 * j)) & 3u];
        }
    });
}

int sahara_synth_reads(const uint8_t* ranks, const uint64_t* rec_lens, uint64_t n_records, uint32_t sigma,
                       uint64_t n_reads, uint32_t len, uint32_t errors, uint64_t seed, uint8_t* out,
                       uint64_t* origin) {
    return guarded([&] { synthReads(ranks, rec_lens, n_records, sigma, n_reads, len, 0, 0, 0, errors, seed, out, origin); });
}

int sahara_synth_reads_typed(const uint8_t* ranks, const uint64_t* rec_lens, uint64_t n_records, uint32_t sigma,
                             uint64_t n_reads, uint32_t len, uint32_t substitutions, uint32_t insertions,
                             uint32_t deletions, uint32_t errors, uint64_t seed, uint8_t* out, uint64_t* origin) {
    return guarded([&] {
        synthReads(ranks, rec_lens, n_records, sigma, n_reads, len, substitutions, insertions, deletions, errors, seed,
                   out, origin);
    });
}

int sahara_pack_2bit(const uint8_t* ranks, uint64_t n, uint32_t sigma, int scalar, uint8_t* out, uint32_t* n_pos,
                     uint64_t pos_cap, uint64_t* n_count) {
    int bad = 0;
    const int rc = guarded([&] {
        if (sigma != 5 && sigma != 6) throw Error("sigma must be 5 or 6");
        if (n >= (1ull << 32)) throw Error("at most 2^32 - 1 symbols per chunk");
        std::vector<uint32_t> pos;
        // scalar: 0 the widest the host has (AVX-512 / AVX2), 1 scalar, 2 AVX2 at most
        const uint64_t acc = scalar == 1 ? pack2Scalar(ranks, out, n, sigma, 0, pos)
                             : scalar == 2 ? (hostHasAvx2() ? pack2Avx2(ranks, out, n, sigma, 0, pos)
                                                            : pack2Scalar(ranks, out, n, sigma, 0, pos))
                                           : pack2Best(ranks, out, n, sigma, 0, pos);
        bad = acc ? 1 : 0;
        *n_count = pos.size();
        if (n_pos && !pos.empty()) std::memcpy(n_pos, pos.data(), std::min<uint64_t>(pos.size(), pos_cap) * 4);
    });
    return rc ? rc : bad;
}

int sahara_interleave_rc(const uint8_t* reads, uint64_t n_reads, uint32_t len, uint32_t sigma, uint8_t* out) {
    return guarded([&] {
        if (sigma != 5 && sigma != 6) throw Error("sigma must be 5 or 6");
        uint8_t comp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (sigma == 6) { comp[1] = 5; comp[2] = 3; comp[3] = 2; comp[4] = 4; comp[5] = 1; }
        else            { comp[1] = 4; comp[2] = 3; comp[3] = 2; comp[4] = 1; }
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint8_t* r = reads + i * len;
            uint8_t* f = out + (2 * i) * len;
            uint8_t* b = out + (2 * i + 1) * len;
            std::memcpy(f, r, len);
            for (uint32_t j = 0; j < len; ++j) b[j] = comp[r[len - 1 - j] & 7];
        }
    });
}

int sahara_cigar(const sahara_alignment* a, uint32_t len, char* buf, size_t cap) {
    if (!a || !buf || a->err == SAHARA_ALIGN_NONE || a->err > SAHARA_ALIGN_MAX_ERR) return -1;
    size_t at = 0;
    char op = 0;
    uint64_t run = 0;
    bool full = false;
    auto flush = [&] {
        if (!run) return;
        char tmp[24];
        const int k = std::snprintf(tmp, sizeof tmp, "%llu%c", (unsigned long long)run, op);
        if (at + (size_t)k + 1 > cap) full = true;
        else std::memcpy(buf + at, tmp, (size_t)k), at += (size_t)k;
        run = 0;
    };
    auto put = [&](char o, uint64_t n) {
        if (!n) return;
        if (o != op) flush();
        op = o;
        run += n;
    };
    uint32_t i = 0;  // pattern symbols written so far
    for (uint32_t s = 0; s < a->err; ++s) {
        const uint32_t qpos = a->edit[s] >> 2, kind = a->edit[s] & 3u;
        if (qpos < i || qpos > len || kind == 0) return -1;
        put('=', qpos - i);
        i = qpos;
        put(kind == 1 ? 'X' : kind == 2 ? 'I' : 'D', 1);
        if (kind != 3) ++i;
    }
    if (i > len) return -1;
    put('=', len - i);
    flush();
    if (full || at + 1 > cap) return -1;
    buf[at] = 0;
    return (int)at;
}

}  // extern "C"
