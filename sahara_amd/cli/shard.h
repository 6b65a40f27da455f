// shard.h — how `sahara search --gpus N` splits the query list over devices, and one device's share of the call.
//
// The reference builds one query list (search.cpp:111-127): per read its
// forward pattern and, unless --no-reverse, its reverse complement, then cuts
// the list at --limit_queries. Device g gets a contiguous range of reads, so
// a read and its reverse complement stay on one device and the qids of all
// devices concatenate in order; sahara_gpu_search_reads cuts
// its own share of the list at `limit`.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "options.h"
#include "output.h"

namespace sahara_cli {

struct QueryShard {
    size_t r0 = 0, r1 = 0;  // reads [r0, r1)
    size_t q0 = 0, q1 = 0;  // their queries [q0, q1) of the interleaved list: qid offset q0, limit q1 - q0
};

// nq = queries after the cut, per = patterns per read (2 with reverse complements, else 1);
// granularity: the reads that stay on one device together (--paired: 2, a pair's mates; the
// shards then split at multiples of it)
inline QueryShard queryShard(size_t nq, size_t per, unsigned devices, unsigned g, size_t granularity = 1) {
    const size_t nreads = (nq + per - 1) / per;  // reads that contribute a query
    const size_t ngroups = (nreads + granularity - 1) / granularity;
    QueryShard s;
    s.r0 = std::min(nreads, ngroups * g / devices * granularity);
    s.r1 = std::min(nreads, ngroups * (g + 1) / devices * granularity);
    s.q0 = std::min(nq, per * s.r0);
    s.q1 = std::min(nq, per * s.r1);
    return s;
}

// Expanded searches, len entries of pi, l, u each. besthits: the schemes of the exact error counts 0..k back to
// back, `counts` holding each one's searches (sahara_gpu_search_best's form); else `counts` is empty.
struct Scheme {
    std::vector<uint32_t> pi, l, u, counts;
    uint32_t n = 0;
};

struct ShardResult {
    HitPart part;
    uint64_t hits = 0;
    double locate = 0, search = 0, align = 0;  // seconds
    std::string err;
    sahara_loci_stats loci{};
    sahara_pairs_stats pairs{};
    sahara_rescue_stats rescue{};
    sahara_best_pairs_stats best{};
    sahara_pair_links_stats links{};
    PairSummaries summary;  // --pair-summary
};

// The stages that the options switch on. Every shard's context gets them: shards split by query and at whole
// pairs, so a locus, a pair, a rescue window and a link each lie within one shard.
inline void configure(void* ctx, const SearchOptions& o) {
    if (o.fmOnly) check(sahara_gpu_set_mode(ctx, 0, 0), "set mode");
    if (o.lociOn) check(sahara_gpu_set_loci(ctx, 1, (uint32_t)o.lociW), "set loci");
    if (o.paired) check(sahara_gpu_set_pairs(ctx, 1, (uint32_t)o.fragLo, (uint32_t)o.fragHi), "set pairs");
    if (o.rescue) check(sahara_gpu_set_rescue(ctx, 1, (uint32_t)o.rescueK, (uint32_t)o.rescueA), "set rescue");
    if (o.bestPairs) check(sahara_gpu_set_best_pairs(ctx, 1, (uint32_t)o.bestDelta), "set best pairs");
    if (o.sam) check(sahara_gpu_set_pair_links(ctx, 1), "set pair links");
}

// The four search calls on a shard's reads, stream symbols [r0 * len, r1 * len) of the codes: all or besthits
// (the schemes as rounds on the device), compact records (8 B each straight into host memory, decoded by the
// writers) or whole ones (--max_hits, a multi-part index).
inline HitPart searchShard(void* ctx, const SearchOptions& o, const PackedReads& R, uint32_t len, const Scheme& S,
                           bool compactOut, const QueryShard& sh) {
    const uint64_t sym0 = (uint64_t)sh.r0 * len, rows = sh.r1 - sh.r0, npat = sh.q1 - sh.q0;
    const uint32_t cap = (uint32_t)std::max(0L, o.maxHits), nc = (uint32_t)S.counts.size();
    const int rc = o.reverse ? 1 : 0, edit = o.edit ? 1 : 0;
    HitPart part;
    int err;
    if (compactOut && o.besthits)
        err = sahara_gpu_search_best_packed_compact(ctx, R.codes, sym0, R.npos, R.ncount, rows, len, rc, npat, S.pi.data(),
                                                    S.l.data(), S.u.data(), S.counts.data(), nc, &part.blocks);
    else if (compactOut)
        err = sahara_gpu_search_packed_compact(ctx, R.codes, sym0, R.npos, R.ncount, rows, len, rc, npat, S.pi.data(),
                                               S.l.data(), S.u.data(), S.n, edit, &part.blocks);
    else if (o.besthits)
        err = sahara_gpu_search_best_packed(ctx, R.codes, sym0, R.npos, R.ncount, rows, len, rc, npat, S.pi.data(),
                                            S.l.data(), S.u.data(), S.counts.data(), nc, cap, &part.hits, &part.n);
    else
        err = sahara_gpu_search_packed(ctx, R.codes, sym0, R.npos, R.ncount, rows, len, rc, npat, S.pi.data(), S.l.data(),
                                       S.u.data(), S.n, edit, cap, &part.hits, &part.n);
    if (err != 0) throw CliError(sahara_gpu_last_error());
    part.compact = compactOut;
    if (compactOut) part.n = part.blocks.n_hits;
    part.qidOffset = sh.q0;
    return part;
}

// --emit-cigar, --sam: the shard's hits aligned on its own device, before the merge. besthits searches with
// edit operations whatever -d says, so its hits align with them too.
inline void alignShard(void* ctx, const SearchOptions& o, const PackedReads& R, uint32_t len, uint32_t sigma,
                       const QueryShard& sh, HitPart& part) {
    const uint64_t sym0 = (uint64_t)sh.r0 * len, rows = sh.r1 - sh.r0, npat = sh.q1 - sh.q0;
    const int rc = o.reverse ? 1 : 0, edit = o.edit || o.besthits ? 1 : 0;
    part.aln.resize(part.n);
    int err;
    if (part.compact) {
        err = sahara_gpu_align_packed_compact(ctx, R.codes, sym0, R.npos, R.ncount, rows, len, rc, npat, edit, o.alignK,
                                              &part.blocks, part.aln.data());
    } else {
        // whole records: the shard's patterns as one rank per byte, the form sahara_gpu_align takes: its reads
        // interleaved with their reverse complements (if searched) and cut to npat, as the search call forms them
        const uint8_t rankOf[5] = {1, 2, 3, (uint8_t)(sigma == 6 ? 5 : 4), 4};
        std::vector<uint8_t> pats(rows * len);
        R.forEach(sym0, pats.size(), [&](uint64_t i, unsigned code) { pats[i] = rankOf[code]; });
        if (rc) {
            std::vector<uint8_t> both(2 * pats.size());
            check(sahara_interleave_rc(pats.data(), rows, len, sigma, both.data()), "interleaving reverse complements");
            pats.swap(both);
        }
        pats.resize(npat * len);
        err = sahara_gpu_align(ctx, pats.data(), npat, len, edit, o.alignK, part.hits, part.n, part.aln.data());
    }
    if (err != 0) throw CliError(sahara_gpu_last_error());
}

// search + locate (src/sahara/search.cpp:218-250) of one shard on its context, then what the call left there
// besides its hits (the stages' statistics, the pairs' summaries, the hits' links) and the alignments; a
// failure is the result's err
inline ShardResult runShard(void* ctx, const SearchOptions& o, const PackedReads& R, uint32_t len, uint32_t sigma,
                            const Scheme& S, bool compactOut, const QueryShard& sh) {
    ShardResult r;
    if (sh.r0 == sh.r1) return r;
    try {
        const StopWatch t0;
        r.part = searchShard(ctx, o, R, len, S, compactOut, sh);
        r.hits = r.part.n;
        sahara_stats st{};
        sahara_gpu_stats(ctx, &st);
        r.locate = (st.locate_ms + st.sort_ms) / 1e3;
        if (o.lociOn) sahara_gpu_loci_stats(ctx, &r.loci);
        if (o.paired) sahara_gpu_pairs_stats(ctx, &r.pairs);
        if (o.rescue) sahara_gpu_rescue_stats(ctx, &r.rescue);
        if (o.bestPairs) sahara_gpu_best_pairs_stats(ctx, &r.best);
        uint64_t got = 0;
        if (o.bestPairs && o.pairSummary) {
            r.summary.rows.resize((sh.q1 - sh.q0) / 4);
            r.summary.pair0 = sh.q0 / 4;
            if (sahara_gpu_pair_summary(ctx, r.summary.rows.data(), r.summary.rows.size(), &got) != 0 ||
                got != r.summary.rows.size())
                throw CliError(std::string("pair summary: ") + sahara_gpu_last_error());
        }
        if (o.sam) {
            r.part.links.resize(r.hits);
            if (sahara_gpu_pair_links(ctx, r.part.links.data(), r.hits, &got) != 0 || got != r.hits)
                throw CliError(std::string("pair links: ") + sahara_gpu_last_error());
            sahara_gpu_pair_links_stats(ctx, &r.links);
        }
        r.search = t0.peek();
        if (o.align && r.hits) {
            const StopWatch tA;
            alignShard(ctx, o, R, len, sigma, sh, r.part);
            r.align = tA.peek();
        }
    } catch (const std::exception& ex) {
        r.err = ex.what();
    }
    return r;
}

}  // namespace sahara_cli
