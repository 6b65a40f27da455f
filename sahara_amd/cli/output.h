// output.h — what `sahara search` writes: the hit lines, the SAM file and the pair summary, from the shards'
// hits as the library hands them over; and the reads as the ingest packs them, which the SAM file quotes.
#pragma once
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../csrc/compact_hit.h"
#include "../csrc/fasta.h"
#include "options.h"

namespace sahara_cli {
using namespace sahara_io;

// The ingest's reads: two bits per symbol (A C G T = 0 1 2 3), back to back, the positions that hold an N
// listed apart in ascending order (npos may be null when ncount is 0).
struct PackedReads {
    const uint8_t* codes;
    const uint64_t* npos;
    uint64_t ncount;
    // f(j, code) for the symbols s0 + j, j in [0, n): the symbol's two bits, or 4 for an N
    template <typename F>
    void forEach(uint64_t s0, uint64_t n, F&& f) const {
        const uint64_t* end = npos + ncount;
        const uint64_t* b = ncount ? std::lower_bound(npos, end, s0) : end;
        for (uint64_t j = 0, s = s0; j < n; ++j, ++s) {
            const bool isN = b != end && *b == s;
            b += isN;
            f(j, isN ? 4u : (unsigned)(codes[s >> 2] >> (2 * (s & 3))) & 3u);
        }
    }
};

// One device's hits: qids local to its shard. Either whole records (hits) or compact ones (blocks,
// sahara_hit_blocks). Owns them: move-only, released with the part.
struct HitPart {
    sahara_hit* hits = nullptr;
    sahara_hit_blocks blocks{};
    bool compact = false;
    uint64_t n = 0;
    uint64_t qidOffset = 0;
    std::vector<sahara_alignment> aln;    // --emit-cigar: record i of hit i, aligned by the hit's own device
    std::vector<sahara_pair_link> links;  // --sam: link i of hit i, relative within the shard
    HitPart() = default;
    HitPart(HitPart&& o) noexcept { *this = std::move(o); }
    HitPart& operator=(HitPart&& o) noexcept {
        release();
        hits = std::exchange(o.hits, nullptr);
        blocks = std::exchange(o.blocks, {});
        compact = std::exchange(o.compact, false);
        n = std::exchange(o.n, 0);
        qidOffset = o.qidOffset;
        aln = std::move(o.aln);
        links = std::move(o.links);
        return *this;
    }
    ~HitPart() { release(); }
    void release() {
        if (compact) sahara_gpu_free_blocks(&blocks);
        else sahara_gpu_free(hits);
        hits = nullptr;
        compact = false;
    }
};

constexpr uint64_t kHitsPerBlock = 1u << 18;   // writeHits (~7 MB of text)
constexpr uint64_t kPairsPerBlock = 1u << 14;  // writeSam (>= 2 lines each)

// The parallel writer: nblocks blocks of text, formatted by nt threads, each
// taking the next block in order (format(bi, buf) fills buf and returns the
// bytes it used). A block's file offset is the previous block's end,
// published as soon as that block is formatted, so each thread writes its own
// block (pwrite) while the others format theirs: formatting and writing both
// run on every thread.
template <typename Format>
void writeBlocks(const std::string& path, size_t nblocks, unsigned nt, Format&& format) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw CliError("can not open output file " + path);
    struct CloseFd {  // closed on every path out (formatting may throw, e.g. bad_alloc)
        int fd;
        bool closed = false;
        int close() { closed = true; return ::close(fd); }
        ~CloseFd() { if (!closed) (void)::close(fd); }
    } closer{fd};
    std::vector<std::atomic<int64_t>> ends(nblocks);
    for (auto& e : ends) e.store(-1, std::memory_order_relaxed);
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    parallelFor(nt, nt, [&](size_t) {
        std::vector<char> buf;
        for (;;) {
            const size_t bi = next.fetch_add(1, std::memory_order_relaxed);
            if (bi >= nblocks) return;
            // A block that fails to format still publishes its end (as an
            // empty block), so that the blocks after it do not wait forever;
            // the call then fails.
            int64_t size = 0;
            try {
                size = (int64_t)format(bi, buf);
            } catch (...) {
                failed.store(true);
                size = 0;
            }
            int64_t off = 0;
            if (bi > 0)
                while ((off = ends[bi - 1].load(std::memory_order_acquire)) < 0) std::this_thread::yield();
            ends[bi].store(off + size, std::memory_order_release);
            for (int64_t done = 0; done < size && !failed.load(std::memory_order_relaxed);) {
                const ssize_t w = ::pwrite(fd, buf.data() + done, (size_t)(size - done), off + done);
                if (w <= 0) failed.store(true);
                else done += w;
            }
        }
    });
    if (closer.close() != 0 || failed.load()) throw CliError("can not write output file " + path);
}

// f(k, hit) for the hits [lo, hi) of a part as whole records with the call's
// qids; compact records are decoded on the way (csrc/compact_hit.h)
template <typename F>
void forEachHit(const HitPart& P, uint64_t lo, uint64_t hi, F&& f) {
    if (!P.compact) {
        for (uint64_t k = lo; k < hi; ++k) {
            const sahara_hit& h = P.hits[k];
            f(k, sahara_hit{h.qid + P.qidOffset, h.seq_id, h.err, h.pos});
        }
        return;
    }
    if (lo >= hi) return;
    const sahara_hit_blocks& H = P.blocks;
    sahara_compact::BlockCursor blk(H.block_end, H.block_qid0, H.n_blocks, lo);
    sahara_compact::RecordCursor rec(H.rec_starts, H.n_records + 1);
    for (uint64_t k = lo; k < hi; ++k) {
        const uint64_t v = H.recs[k], pos = rec.seek(sahara_compact::textOf(v));
        f(k, sahara_hit{blk.qid0Of(k) + sahara_compact::qidOf(v) + P.qidOffset, (uint32_t)rec.seq,
                        sahara_compact::errOf(v), pos});
    }
}

// Text output of hits: "qid seqId pos[ e][ cigar]\n" (search.cpp:254-261; the CIGAR of patterns of cigarLen
// symbols when the parts carry alignments), formatted and written by nt threads in blocks of blockHits hits.
inline void writeHits(const std::string& path, const std::vector<HitPart>& parts, bool emitErrors, unsigned nt,
                      uint32_t cigarLen = 0, uint64_t blockHits = kHitsPerBlock) {
    struct Block {
        const HitPart* part;
        uint64_t lo, hi;
    };
    std::vector<Block> blocks;
    for (const auto& hp : parts)
        for (uint64_t lo = 0; lo < hp.n; lo += blockHits) blocks.push_back({&hp, lo, std::min(hp.n, lo + blockHits)});
    writeBlocks(path, blocks.size(), nt, [&](size_t bi, std::vector<char>& buf) {
        const Block& B = blocks[bi];
        buf.resize((B.hi - B.lo) * (cigarLen ? 256 : 96));
        char* o = buf.data();
        char* e = o + buf.size();
        const HitPart& P = *B.part;
        forEachHit(P, B.lo, B.hi, [&](uint64_t k, const sahara_hit& h) {
            auto num = [&](uint64_t v, char after) {
                o = std::to_chars(o, e, v).ptr;
                *o++ = after;
            };
            num(h.qid, ' ');
            num(h.seq_id, ' ');
            num(h.pos, emitErrors || cigarLen ? ' ' : '\n');
            if (emitErrors) num(h.err, cigarLen ? ' ' : '\n');
            if (!cigarLen) return;
            const int n = sahara_cigar(&P.aln[k], cigarLen, o, (size_t)(e - o));  // (at most 8 edits: < 150 characters)
            if (n >= 0) o += n;
            else *o++ = '*';  // no alignment within the bound
            *o++ = '\n';
        });
        return (size_t)(o - buf.data());
    });
}

// The reads of a --sam call: read r at symbol r * len.
struct SamReads {
    PackedReads reads;
    uint32_t len;
    void pattern(uint64_t qid, char* out) const {  // qid's letters (read qid / 2; odd: its reverse complement)
        const bool rc = qid & 1;
        reads.forEach((qid >> 1) * len, len, [&](uint64_t j, unsigned c) {
            if (rc) out[len - 1 - j] = "TGCAN"[c];
            else out[j] = "ACGTN"[c];
        });
    }
};

// --sam (docs/semantics.md "SAM output"): the kept hits of a --best-pairs search as SAM records, a line per
// hit, from the shards' hits (compact records), links and alignments; a pair that keeps nothing writes its two
// reads unmapped. Names are numbers: QNAME the pair, RNAME the record. The pairs are written in query order
// in blocks of blockPairs pairs.
inline void writeSam(const std::string& path, const std::vector<HitPart>& parts, const SamReads& R, uint64_t npairs,
                     unsigned nt, uint64_t blockPairs = kPairsPerBlock) {
    const sahara_hit_blocks* any = nullptr;
    for (const auto& hp : parts)
        if (hp.compact) any = &hp.blocks;
    if (!any) throw CliError("--sam: no shard returned compact records");
    // the shards' hits as whole records (qids of the call), decoded in parallel
    std::vector<std::vector<sahara_hit>> whole(parts.size());
    for (size_t g = 0; g < parts.size(); ++g) {
        const HitPart& P = parts[g];
        if (!P.n) continue;
        if (!P.compact || P.links.size() != P.n || P.aln.size() != P.n)
            throw CliError("--sam: a shard's hits came without links or alignments");
        whole[g].resize(P.n);
        parallelFor(nt, nt, [&](size_t t) {
            forEachHit(P, P.n * t / nt, P.n * (t + 1) / nt, [&](uint64_t k, const sahara_hit& h) { whole[g][k] = h; });
        });
    }
    struct Block {
        size_t part;      // the shard that holds the pairs (parts.size(): none of them has a hit there)
        uint64_t p0, p1;  // pairs [p0, p1)
    };
    // the pairs in blocks, cut at the shards' borders: shard g holds the pairs from its qidOffset / 4 up to the next's
    std::vector<Block> blocks;
    {
        uint64_t p = 0;
        auto add = [&](size_t part, uint64_t upTo) {
            for (; p < upTo; p += std::min(blockPairs, upTo - p)) blocks.push_back({part, p, std::min(upTo, p + blockPairs)});
        };
        for (size_t g = 0; g < parts.size(); ++g) {
            if (!parts[g].n) continue;
            add(parts.size(), parts[g].qidOffset / 4);  // (pairs before this shard's first: of shards without a hit)
            uint64_t end = npairs;
            for (size_t h = g + 1; h < parts.size(); ++h)
                if (parts[h].n) {
                    end = parts[h].qidOffset / 4;
                    break;
                }
            add(g, end);
        }
        add(parts.size(), npairs);
    }
    const uint32_t len = R.len;
    writeBlocks(path, blocks.size() + 1, nt, [&](size_t bi, std::vector<char>& buf) {
        buf.clear();
        auto text = [&](const char* s) { buf.insert(buf.end(), s, s + std::strlen(s)); };
        auto num = [&](const char* lead, long long v) {  // lead, then v in decimal
            char b[24];
            const auto r = std::to_chars(b, b + sizeof(b), v);
            text(lead);
            buf.insert(buf.end(), b, r.ptr);
        };
        if (bi == 0) {  // block 0 is the header
            text("@HD\tVN:1.6\tSO:unsorted\tGO:query\n");
            for (uint64_t r = 0; r < any->n_records; ++r) {
                num("@SQ\tSN:", (long long)r);
                num("\tLN:", (long long)(any->rec_starts[r + 1] - any->rec_starts[r] - 1));
                text("\n");
            }
            text("@PG\tID:sahara\tPN:sahara\n");
            return buf.size();
        }
        const Block& B = blocks[bi - 1];
        std::vector<char> seq(len);
        auto pattern = [&](uint64_t qid) {
            R.pattern(qid, seq.data());
            buf.insert(buf.end(), seq.begin(), seq.end());
        };
        const std::vector<sahara_hit>* W = B.part < parts.size() ? &whole[B.part] : nullptr;
        uint64_t k = 0;
        if (W) k = (uint64_t)(std::lower_bound(W->begin(), W->end(), 4 * B.p0,
                                               [](const sahara_hit& h, uint64_t q) { return h.qid < q; }) - W->begin());
        for (uint64_t p = B.p0; p < B.p1; ++p) {
            if (!W || k >= W->size() || (*W)[k].qid >> 2 != p) {  // the pair keeps nothing: its two reads, unmapped
                for (int mate = 0; mate < 2; ++mate) {
                    num("", (long long)p);
                    text(mate ? "\t141\t*\t0\t0\t*\t*\t0\t0\t" : "\t77\t*\t0\t0\t*\t*\t0\t0\t");
                    pattern(4 * p + 2 * mate);
                    text("\t*\n");
                }
                continue;
            }
            const HitPart& P = parts[B.part];
            for (; k < W->size() && (*W)[k].qid >> 2 == p; ++k) {
                const sahara_hit& h = (*W)[k];
                const sahara_pair_link& L = P.links[k];
                const uint64_t km = (uint64_t)((int64_t)k + L.mate);
                if (km >= W->size()) throw CliError("--sam: a link leaves its shard's hits");
                const sahara_hit& m = (*W)[km];
                const sahara_alignment &A = P.aln[k], &Am = P.aln[km];
                const bool none = A.err == SAHARA_ALIGN_NONE, noneM = Am.err == SAHARA_ALIGN_NONE;
                const uint64_t end = h.pos + (none ? len : A.ref_len), endM = m.pos + (noneM ? len : Am.ref_len);
                const long long span = (long long)(std::max(end, endM) - std::min(h.pos, m.pos));
                const bool left = h.pos < m.pos || (h.pos == m.pos && (h.qid & 1) == 0);
                const unsigned flag = 0x1u | 0x2u | ((h.qid & 1) ? 0x10u : 0x20u) | ((h.qid & 2) ? 0x80u : 0x40u) |
                                      ((L.flags & SAHARA_LINK_PRIMARY) ? 0u : 0x100u);
                num("", (long long)p);
                num("\t", flag);
                num("\t", h.seq_id);
                num("\t", (long long)h.pos + 1);
                num("\t", L.mapq);
                text("\t");
                char cg[16 * (SAHARA_ALIGN_MAX_ERR + 2)];
                const int n = sahara_cigar(&A, len, cg, sizeof(cg));
                if (n >= 0) buf.insert(buf.end(), cg, cg + n);
                else text("*");  // no alignment within the bound
                num("\t=\t", (long long)m.pos + 1);
                num("\t", left ? span : -span);
                text("\t");
                pattern(h.qid);
                num("\t*\tNM:i:", none ? (long long)h.err : (long long)A.err);
                num("\tZP:i:", L.score);
                text("\n");
            }
        }
        return buf.size();
    });
}

// --pair-summary: a shard's pairs, the first being pair pair0 of the call; a line "pair best next n_fwd n_rev"
// per pair that keeps a hit, the shards in order
struct PairSummaries {
    std::vector<sahara_pair_summary> rows;
    uint64_t pair0 = 0;
};
inline void writePairSummary(const std::string& path, const std::vector<PairSummaries>& shards) {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) throw CliError("cannot write " + path);
    for (const PairSummaries& s : shards)
        for (size_t i = 0; i < s.rows.size(); ++i) {
            const sahara_pair_summary& x = s.rows[i];
            if (x.best != 255)
                std::fprintf(f, "%llu\t%u\t%u\t%u\t%u\n", (unsigned long long)(s.pair0 + i), x.best, x.next, x.n_fwd,
                             x.n_rev);
        }
    if (std::fclose(f) != 0) throw CliError("cannot write " + path);
}

}  // namespace sahara_cli
