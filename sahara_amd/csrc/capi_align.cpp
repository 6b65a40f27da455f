// capi_align.cpp — the alignment calls of the C ABI (include/sahara_hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "align.h"
#include "ctx.h"

using namespace sahara;

// sahara_gpu_align[_packed_compact]: the call's patterns staged whole as
// 3-bit-plane blocks, then the hit records up and the alignment records down
// chunk by chunk on stream st, kAlignHits between (align.hip). Every hit is
// checked on the host before anything is staged: a refused call launches
// nothing and leaves `out` alone.

static void checkAlignBounds(uint32_t len, uint32_t max_err) {
    if (max_err > SAHARA_ALIGN_MAX_ERR)
        throw Error("alignment: max_err above SAHARA_ALIGN_MAX_ERR (" + std::to_string(SAHARA_ALIGN_MAX_ERR) + ")");
    if (len == 0 || len > 16383) throw Error("alignment: pattern length out of range (1..16383)");
}

static uint64_t alignChunk() {
    const char* e = std::getenv("SAHARA_ALIGN_CHUNK");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? std::min<uint64_t>((uint64_t)v, 1ull << 28) : 1ull << 22;
}

// f(a, b) over [0, n) in slices, on up to 8 threads (the checks of tens of millions of hit records)
static void alignSlices(uint64_t n, const std::function<void(uint64_t, uint64_t)>& f) {
    const unsigned nt = n < (1u << 20) ? 1 : std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    if (nt == 1) return f((uint64_t)0, n);
    const uint64_t per = (n + nt - 1) / nt;
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < nt; ++t) {
        const uint64_t a = std::min(n, t * per), b = std::min(n, a + per);
        if (a < b) ts.emplace_back([&f, a, b] { f(a, b); });
    }
    for (auto& t : ts) t.join();
}

// the patterns [0, npat) of rank bytes -> c->align.pats3
static void alignStageRanks(Ctx* c, const uint8_t* ranks, uint64_t npat, uint32_t m, uint32_t patBlocks) {
    Ctx::Align& A = c->align;
    A.pats3.reserve(npat * patBlocks + 1);
    const uint64_t rowsPer = std::max<uint64_t>(1, (64ull << 20) / m);
    A.raw.reserve(std::min(npat, rowsPer) * m);
    for (uint64_t r0 = 0; r0 < npat; r0 += rowsPer) {
        const uint64_t rows = std::min(rowsPer, npat - r0);
        SH_HIP(hipMemcpyAsync(A.raw.ptr, ranks + r0 * m, rows * m, hipMemcpyHostToDevice, c->st));
        launchPackPatterns3(A.raw.ptr, rows, m, patBlocks, A.pats3.ptr + r0 * patBlocks, c->st);
        SH_HIP(hipStreamSynchronize(c->st));  // (raw is reused)
    }
}

// the query list of a packed-reads call (R, as the search call forms it) -> c->align.pats3
static void alignStagePacked(Ctx* c, const uint8_t* codes, const PackedReads& pk, const ReadRows& R, bool rc,
                             uint32_t m, uint32_t patBlocks) {
    Ctx::Align& A = c->align;
    if (c->I.sigma != 5 && c->I.sigma != 6) throw Error("reads two bits per symbol need a dna4 or dna5 index");
    const uint32_t patWords = (m + 7) / 8;
    A.pats3.reserve(R.npat * patBlocks + 1);
    A.pats4.reserve(R.npat * patWords);
    const uint64_t lo = pk.sym0, hi = pk.sym0 + R.rows * m;
    const uint64_t* nb = pk.nCount ? std::lower_bound(pk.nPos, pk.nPos + pk.nCount, lo) : nullptr;
    const uint64_t* ne = pk.nCount ? std::lower_bound(nb, pk.nPos + pk.nCount, hi) : nullptr;
    for (const uint64_t* q = nb; q && q < ne; ++q)
        if (*q < lo || *q >= hi || (q > nb && *q <= q[-1]))
            throw Error("N positions of packed reads must be strictly ascending");
    if (nb != ne && c->I.sigma == 5) throw Error("pattern rank out of range for this index");
    // chunks of whole reads, an even number each (a read and its reverse
    // complement are patterns of one chunk), < 2^30 symbols: N positions
    // relative to the chunk's first byte fit 32 bits
    uint64_t rowsPer = std::max<uint64_t>(2, ((1ull << 28) / m) & ~1ull);
    A.raw.reserve((std::min(R.rows, rowsPer) * m + 3) / 4 + 64);  // (a chunk's bytes start up to 4 early)
    std::vector<uint32_t> rel;
    for (uint64_t r0 = 0; r0 < R.rows; r0 += rowsPer) {
        const uint64_t r1 = std::min(R.rows, r0 + rowsPer);
        const uint64_t S0 = lo + r0 * m, S1 = lo + r1 * m;
        const uint64_t B0 = (S0 / 4) & ~uint64_t(3), B1 = (S1 + 3) / 4;  // the chunk's bytes, from a whole word on
        SH_HIP(hipMemsetAsync(A.raw.ptr + (B1 - B0), 0, 32, c->st));    // (kPackFrom2 reads three words per block)
        SH_HIP(hipMemcpyAsync(A.raw.ptr, codes + B0, B1 - B0, hipMemcpyHostToDevice, c->st));
        rel.clear();
        for (; nb && nb < ne && *nb < S1; ++nb) rel.push_back((uint32_t)(*nb - 4 * B0));
        A.nList.reserve(std::max<size_t>(rel.size(), 1));
        if (!rel.empty())
            SH_HIP(hipMemcpyAsync(A.nList.ptr, rel.data(), rel.size() * 4, hipMemcpyHostToDevice, c->st));
        const uint64_t p0 = rc ? 2 * r0 : r0, p1 = rc ? std::min(2 * r1, R.npat) : r1;
        launchPackFrom2(A.raw.ptr, (uint32_t)(S0 - 4 * B0), A.nList.ptr, (uint32_t)rel.size(), r0, p0, p1, m, rc,
                        c->I.sigma, patWords, patBlocks, A.pats4.ptr, A.pats3.ptr, c->st);
        SH_HIP(hipStreamSynchronize(c->st));  // (raw, nList and rel are reused)
    }
}

// The chunk loop. recSize: bytes of a hit record (24 whole, 8 compact).
static void alignChunks(Ctx* c, AlignArgs a, const void* hits, size_t recSize, uint64_t n_hits, sahara_alignment* out,
                        double& kernelMs, uint64_t& chunks) {
    Ctx::Align& A = c->align;
    const uint64_t per = alignChunk();
    A.in.reserve(std::min(per, n_hits) * recSize);
    A.out.reserve(std::min(per, n_hits));
    const Event e0(hipEventDefault), e1(hipEventDefault);
    const bool whole = recSize == sizeof(sahara_hit);
    for (uint64_t i0 = 0; i0 < n_hits; i0 += per, ++chunks) {
        const uint64_t n = std::min(per, n_hits - i0);
        SH_HIP(hipMemcpyAsync(A.in.ptr, static_cast<const char*>(hits) + i0 * recSize, n * recSize,
                              hipMemcpyHostToDevice, c->st));
        a.nHits = n;
        a.first = i0;
        a.out = A.out.ptr;
        if (whole) a.hits = reinterpret_cast<const sahara_hit*>(A.in.ptr);
        else a.recs = reinterpret_cast<const uint64_t*>(A.in.ptr);
        SH_HIP(hipEventRecord(e0, c->st));
        for (uint32_t p = 0; p <= c->more.size(); ++p) {  // every hit's record is of exactly one part
            const DeviceIndex& I = partOf(c, p);
            a.text3 = I.text3.ptr;
            a.text3Bytes = (uint32_t)std::min<uint64_t>(text3Blocks(I.n) * 16, 0xFFFFFF00ull);
            a.recStarts = I.dRecStarts.ptr;
            a.rec0 = c->partRec0[p];
            a.nrec = I.recLens.size();
            launchAlignHits(a, c->st);
        }
        SH_HIP(hipEventRecord(e1, c->st));
        SH_HIP(hipStreamSynchronize(c->st));  // (copyOut's small copies are not on st)
        copyOut(c, out + i0, A.out.ptr, n * sizeof(sahara_alignment));
        SH_HIP(hipStreamSynchronize(c->st));
        float ms = 0;
        SH_HIP(hipEventElapsedTime(&ms, e0, e1));
        kernelMs += ms;
    }
}

// What both calls end with: the kernel's arguments that the two record forms
// share (the patterns staged in c->align.pats3), and the call's stats.
using clk = std::chrono::steady_clock;
static double msSince(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

static AlignArgs alignArgs(Ctx* c, uint32_t len, int edit, uint32_t max_err) {
    AlignArgs a{};
    a.pats3 = c->align.pats3.ptr;
    a.patBlocks = (len + 31) / 32;
    a.m = len;
    a.maxErr = max_err;
    a.edit = edit != 0;
    return a;
}

static void alignDone(Ctx* c, sahara_align_stats& S, uint64_t n_hits, clk::time_point t0) {
    S.hits = n_hits;
    S.total_ms = msSince(t0);
    c->align.stats = S;
}

extern "C" {

int sahara_gpu_align(void* ctx, const uint8_t* ranks, uint64_t n_patterns, uint32_t len, int edit, uint32_t max_err,
                     const sahara_hit* hits, uint64_t n_hits, sahara_alignment* out) {
    return guarded([&] {
        const auto t0 = clk::now();
        Ctx* c = ctxOf(ctx);
        checkAlignBounds(len, max_err);
        if (n_hits && (!hits || !out || !ranks)) throw Error("sahara_gpu_align: null input");
        // the hit records alone, before any address is formed from them
        std::vector<const std::vector<uint64_t>*> lens;  // per part
        for (uint32_t p = 0; p <= c->more.size(); ++p) lens.push_back(&partOf(c, p).recLens);
        const uint64_t nrec = c->partRec0.back() + lens.back()->size();
        std::atomic<uint64_t> firstBad{UINT64_MAX};  // the first hit that fails a check
        alignSlices(n_hits, [&](uint64_t a, uint64_t b) {
            uint32_t part = 0;
            for (uint64_t i = a; i < b; ++i) {
                const sahara_hit& h = hits[i];
                bool ok = h.qid < n_patterns && h.seq_id < nrec;
                if (ok) {
                    if (h.seq_id < c->partRec0[part] || h.seq_id - c->partRec0[part] >= lens[part]->size())
                        part = (uint32_t)(std::upper_bound(c->partRec0.begin(), c->partRec0.end(),
                                                           (uint64_t)h.seq_id) - c->partRec0.begin() - 1);
                    ok = h.pos < (*lens[part])[h.seq_id - c->partRec0[part]];
                }
                if (!ok) {
                    uint64_t seen = firstBad.load();
                    while (i < seen && !firstBad.compare_exchange_weak(seen, i)) {}
                    return;
                }
            }
        });
        if (const uint64_t i = firstBad.load(); i != UINT64_MAX) {
            const sahara_hit& h = hits[i];
            if (h.qid >= n_patterns)
                throw Error("sahara_gpu_align: hit " + std::to_string(i) + " names pattern " + std::to_string(h.qid) +
                            " of " + std::to_string(n_patterns));
            if (h.seq_id >= nrec)
                throw Error("sahara_gpu_align: hit " + std::to_string(i) + " names record " +
                            std::to_string(h.seq_id) + " of " + std::to_string(nrec));
            throw Error("sahara_gpu_align: hit " + std::to_string(i) + " lies at position " + std::to_string(h.pos) +
                        " outside record " + std::to_string(h.seq_id));
        }
        sahara_align_stats S{};
        if (n_hits) {
            const uint32_t patBlocks = (len + 31) / 32;
            alignStageRanks(c, ranks, n_patterns, len, patBlocks);
            S.stage_ms = msSince(t0);
            alignChunks(c, alignArgs(c, len, edit, max_err), hits, sizeof(sahara_hit), n_hits, out, S.kernel_ms, S.chunks);
        }
        alignDone(c, S, n_hits, t0);
    });
}

int sahara_gpu_align_packed_compact(void* ctx, const uint8_t* codes, uint64_t sym0, const uint64_t* n_pos,
                                    uint64_t n_count, uint64_t n_reads, uint32_t len, int reverse, uint64_t limit,
                                    int edit, uint32_t max_err, const sahara_hit_blocks* blocks, sahara_alignment* out) {
    return guarded([&] {
        const auto t0 = clk::now();
        Ctx* c = ctxOf(ctx);
        checkAlignBounds(len, max_err);
        if (!c->more.empty()) throw Error("compact hit records need a single-part index (text < 2^32 symbols)");
        if (!blocks || !codes || (n_count && !n_pos)) throw Error("sahara_gpu_align_packed_compact: null input");
        const ReadRows R = readRows(reverse, n_reads, limit);
        const uint64_t n_hits = blocks->n_hits;
        if (n_hits && (!blocks->recs || !blocks->block_end || !blocks->block_qid0 || !blocks->n_blocks || !out))
            throw Error("sahara_gpu_align_packed_compact: null input");
        if (blocks->n_blocks > 0xFFFFFFFFull) throw Error("sahara_gpu_align_packed_compact: too many blocks");
        // the records alone: blocks in order and covering them, every qid a pattern, every position in the text
        uint64_t covered = 0;
        for (uint64_t b = 0; n_hits && b < blocks->n_blocks; ++b) {
            if (blocks->block_end[b] < covered || blocks->block_end[b] > n_hits)
                throw Error("sahara_gpu_align_packed_compact: block ends out of order");
            covered = blocks->block_end[b];
        }
        if (covered != n_hits) throw Error("sahara_gpu_align_packed_compact: the blocks do not cover the records");
        std::atomic<uint64_t> firstBad{UINT64_MAX};
        alignSlices(n_hits, [&](uint64_t a, uint64_t b) {
            const uint64_t* ends = blocks->block_end;
            uint64_t blk = (uint64_t)(std::upper_bound(ends, ends + blocks->n_blocks, a) - ends);
            for (uint64_t i = a; i < b; ++i) {
                while (i >= ends[blk]) ++blk;
                const uint64_t v = blocks->recs[i], q0 = blocks->block_qid0[blk];
                if (q0 >= R.npat || (v >> 36) >= R.npat - q0 || ((v >> 4) & 0xFFFFFFFFull) >= c->I.n) {
                    uint64_t seen = firstBad.load();
                    while (i < seen && !firstBad.compare_exchange_weak(seen, i)) {}
                    return;
                }
            }
        });
        if (const uint64_t i = firstBad.load(); i != UINT64_MAX) {
            if (((blocks->recs[i] >> 4) & 0xFFFFFFFFull) >= c->I.n)
                throw Error("sahara_gpu_align_packed_compact: record " + std::to_string(i) + " lies outside the text");
            throw Error("sahara_gpu_align_packed_compact: record " + std::to_string(i) +
                        " names a pattern beyond the " + std::to_string(R.npat) + " of the call");
        }
        sahara_align_stats S{};
        if (n_hits) {
            const uint32_t patBlocks = (len + 31) / 32;
            const PackedReads pk{sym0, n_pos, n_count};
            alignStagePacked(c, codes, pk, R, reverse != 0, len, patBlocks);
            Ctx::Align& A = c->align;
            const uint64_t nb = blocks->n_blocks;
            A.blocks.reserve(2 * nb);
            SH_HIP(hipMemcpyAsync(A.blocks.ptr, blocks->block_end, nb * 8, hipMemcpyHostToDevice, c->st));
            SH_HIP(hipMemcpyAsync(A.blocks.ptr + nb, blocks->block_qid0, nb * 8, hipMemcpyHostToDevice, c->st));
            SH_HIP(hipStreamSynchronize(c->st));
            S.stage_ms = msSince(t0);
            AlignArgs a = alignArgs(c, len, edit, max_err);
            a.blockEnd = A.blocks.ptr;
            a.blockQid0 = A.blocks.ptr + nb;
            a.nBlocks = (uint32_t)nb;
            alignChunks(c, a, blocks->recs, 8, n_hits, out, S.kernel_ms, S.chunks);
        }
        alignDone(c, S, n_hits, t0);
    });
}

int sahara_gpu_align_stats(void* ctx, sahara_align_stats* stats) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!stats) throw Error("sahara_gpu_align_stats: null output");
        *stats = c->align.stats;
    });
}

}  // extern "C"
