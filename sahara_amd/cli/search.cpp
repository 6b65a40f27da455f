// search.cpp — `sahara search` (src/sahara/search.cpp:22-291; "search.cpp:n" below is that file) as a sequence of
// steps: options (options.h); index load beside the query ingest; scheme; a run per shard (shard.h); output (output.h); stats.

#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <fcntl.h>
#include <fstream>
#include <future>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

#include "../csrc/fasta.h"
#include "options.h"
#include "output.h"
#include "shard.h"

namespace sahara_cli {
using namespace sahara_io;

namespace {

// A read-only mapping of a whole file (the .idx image every device loads).
struct MappedFile {
    const void* data = nullptr;
    size_t size = 0;
    explicit MappedFile(const std::string& path) {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw CliError("no valid index path at " + path);
        struct stat sb {};
        if (::fstat(fd, &sb) != 0 || sb.st_size == 0) {
            ::close(fd);
            throw CliError("can not read index " + path);
        }
        size = (size_t)sb.st_size;
        void* p = ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (p == MAP_FAILED) throw CliError("can not map index " + path);
        (void)::madvise(p, size, MADV_WILLNEED);
        data = p;
    }
    ~MappedFile() {
        if (data) ::munmap(const_cast<void*>(data), size);
    }
    MappedFile(const MappedFile&) = delete;
};

// Reads in a FASTA file and their length, estimated from its first 256 KB
// and its size (sahara_gpu_prepare's sizes; 0 when unknown). Errs high.
struct QueryEstimate {
    uint64_t reads = 0;
    uint32_t len = 0;
};
QueryEstimate estimateQueries(const std::string& path) {
    QueryEstimate q;
    struct stat sb {};
    if (::stat(path.c_str(), &sb) != 0 || sb.st_size <= 0) return q;
    std::ifstream f(path, std::ios::binary);
    std::vector<char> buf(256u << 10);
    f.read(buf.data(), (std::streamsize)buf.size());
    const size_t n = (size_t)f.gcount();
    std::vector<size_t> heads;  // '>' at line starts
    for (size_t i = 0; i < n; ++i)
        if (buf[i] == '>' && (i == 0 || buf[i - 1] == '\n')) heads.push_back(i);
    if (heads.size() < 2) return q;
    const double perRec = (double)(heads.back() - heads[0]) / (double)(heads.size() - 1);
    size_t i = heads[0];
    while (i < heads[1] && buf[i] != '\n') ++i;  // the first header line
    for (; i < heads[1]; ++i)
        if (buf[i] != '\n' && buf[i] != '\r') ++q.len;
    q.reads = (uint64_t)((double)sb.st_size / perRec * 1.05) + 16;
    return q;
}

uint64_t readSigma(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw CliError("no valid index path at " + path);
    uint64_t s = 0;
    f.read(reinterpret_cast<char*>(&s), 8);
    if (!f) throw CliError("can not read index " + path);
    return s;
}

// Index residency (search.cpp:162-169): one context per device, the devices loading the one mapped .idx image
// side by side, beside the query ingest (host threads there, DMA here). The search call's one-time work happens
// here too (sahara_gpu_prepare, sized by an estimate of the queries): the hit sink is pinned while the index loads,
// the pass's buffers are made once it is resident. Compact records only, <= 2 devices (the pool keeps two sinks).
struct IndexLoad {
    MappedFile img;
    std::vector<void*> ctx;
    std::vector<double> seconds;  // each device's whole load
    std::vector<std::string> errs;
    std::shared_future<void> pinned;
    std::vector<std::thread> th;
    explicit IndexLoad(const SearchOptions& o) : img(o.index), ctx(o.ngpu, nullptr), seconds(o.ngpu, 0.0), errs(o.ngpu) {}
    void start(const SearchOptions& o) {
        if (!o.limitError.empty()) throw CliError(o.limitError);
        const QueryEstimate qe = o.maxHits <= 0 && o.ngpu <= 2 ? estimateQueries(o.query) : QueryEstimate{};
        uint64_t npatEst = (o.reverse ? 2 : 1) * qe.reads;
        npatEst = std::min<uint64_t>(npatEst, o.limit);
        npatEst = (npatEst + o.ngpu - 1) / o.ngpu + 2;
        if (qe.reads)
            pinned = std::async(std::launch::async, [npatEst] { (void)sahara_gpu_prepare(nullptr, npatEst, 0); }).share();
        const StopWatch sw;
        for (uint32_t g = 0; g < o.ngpu; ++g)
            th.emplace_back([this, g, qe, npatEst, sw] {
                if (sahara_gpu_open((int)g, img.data, img.size, &ctx[g]) != 0) errs[g] = sahara_gpu_last_error();
                seconds[g] = sw.peek();
                if (qe.reads && ctx[g]) {
                    pinned.wait();
                    (void)sahara_gpu_prepare(ctx[g], npatEst, qe.len);  // a failure only costs the call its time
                }
            });
    }
    void join() {
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
    void close() {
        for (void*& c : ctx) sahara_gpu_close(c), c = nullptr;
    }
    ~IndexLoad() {  // also on an exception: the contexts close after their loads end
        join();
        close();
    }
};

// Queries (search.cpp:111-130): the library's ingest (sahara_read_fasta) parses and verifies them straight into
// PackedReads' form in page-locked memory, which the search calls DMA without a copy; the reverse complements and
// the --limit_queries cut are made on the device. Query numbers in messages count the interleaved list.
struct Queries {
    sahara_fasta f{};
    ~Queries() { sahara_free_fasta(&f); }
};

// the interleaved query list's length after --limit_queries; the checks that need the queries
size_t verifyQueries(const SearchOptions& o, const sahara_fasta& f, size_t per) {
    if (f.bad) {
        const unsigned char ch = (unsigned char)f.bad_char;
        throw CliError(fmtStr("query '%s' (%zu) has invalid character at position %ld '%c'(%x)", f.bad_id,
                              per * (size_t)f.bad_record + 1, (long)f.bad_pos, ch, ch));
    }
    size_t nq = per * f.n_records;
    nq = (size_t)std::min<uint64_t>(o.limit, nq);
    if (nq == 0) throw CliError("query file " + o.query + " was empty - abort\n");
    if (!o.paired) return nq;
    if (f.n_records % 2)
        throw CliError("--paired: " + o.query + " holds " + std::to_string(f.n_records) +
                       " reads, an odd number: the mates of a pair come one after the other");
    const uint64_t len0 = f.offs[1] - f.offs[0];
    if (o.fragHi < len0)
        throw CliError("--paired: --max-fragment " + std::to_string(o.fragHi) + " is below the read length " +
                       std::to_string(len0));
    return nq;
}

void checkGenerator(const std::string& gen) {
    const char* names[64];
    int ng = sahara_scheme_generators(names, nullptr, 64);
    // the reference lists generator::all's keys, a map: sorted by name (search.cpp:177-181)
    std::vector<std::string> sorted(names, names + ng);
    std::sort(sorted.begin(), sorted.end());
    bool known = false;
    std::string all;
    for (size_t i = 0; i < sorted.size(); ++i) {
        known = known || gen == sorted[i];
        all += (i ? ", " : "") + sorted[i];
    }
    if (!known) throw CliError("unknown search scheme generetaror \"" + gen + "\", valid generators are: " + all);
}

// fmt's "{}" for a double: shortest round-trip representation
std::string shortest(double v) {
    char b[64];
    auto r = std::to_chars(b, b + sizeof(b), v);
    return std::string(b, r.ptr);
}

// One expansion to the reads' length, for minK..maxK errors, of an index of sigma letters and n symbols.
// --dynamic_generator: part sizes by weighted node count (search.cpp:192-195, 202-205), printed on request.
Scheme expandScheme(const SearchOptions& o, uint32_t len, int sigma, double n, int minK, int maxK, bool hamming,
                    bool printPartition) {
    const char* gen = o.generator.c_str();
    const int ham = hamming ? 1 : 0, edit = o.edit ? 1 : 0;
    std::vector<uint32_t> sizes(64);
    Scheme s;
    auto expand = [&](int h, uint32_t* sz, int cap) {  // into s, or with cap == 0 only the count
        uint32_t *pi = cap ? s.pi.data() : nullptr, *l = cap ? s.l.data() : nullptr, *u = cap ? s.u.data() : nullptr;
        return o.dynamic ? sahara_scheme_dynamic(gen, minK, maxK, len, h, edit, sigma, n, sz, sz ? 64 : 0, pi, l, u, cap)
                         : sahara_scheme(gen, minK, maxK, len, ham, pi, l, u, cap);
    };
    const std::string toLength = " to length " + std::to_string(len);
    const int ns = expand(0, nullptr, 0);
    if (ns < 0) throw CliError("cannot expand search scheme " + o.generator + (o.dynamic ? "" : toLength));
    s.n = (uint32_t)ns;
    s.pi.resize((size_t)ns * len), s.l.resize((size_t)ns * len), s.u.resize((size_t)ns * len);
    if (expand(ham, sizes.data(), ns) != ns) throw CliError("cannot expand search scheme " + o.generator + toLength);
    if (o.dynamic && printPartition) {
        int P = 0;
        sahara_scheme_parts(gen, minK, maxK, &P, nullptr, nullptr, nullptr, 0);
        std::string part = "[";
        for (int i = 0; i < P; ++i) part += (i ? ", " : "") + std::to_string(sizes[i]);
        std::printf("partition: %s]\n", part.c_str());
    }
    return s;
}

// The scheme the call searches (search.cpp:174-212). all: errors 0..k; besthits: one per exact error count,
// back to back. Each expansion's node counts are printed right after it, as loadSearchScheme prints them
// (search.cpp:186-212): on the expanded scheme, before limitToHamming.
Scheme searchedScheme(const SearchOptions& o, uint32_t len, int sigma, double n) {
    auto counted = [&](int minK, int maxK) {
        Scheme s = expandScheme(o, len, sigma, n, minK, maxK, false, true);
        double nc = 0, wnc = 0;
        sahara_scheme_counts(s.l.data(), s.u.data(), s.n, len, o.edit ? 1 : 0, sigma, n, &nc, &wnc);
        std::printf("node count: %s\nweighted node count: %s\n", shortest(nc).c_str(), shortest(wnc).c_str());
        return s;
    };
    if (!o.besthits) {
        Scheme s = counted(0, o.k);
        // -d ham: the search runs on limitToHamming of that scheme (search.cpp:226)
        return o.edit ? s : expandScheme(o, len, sigma, n, 0, o.k, true, false);
    }
    Scheme all;
    for (int j = 0; j <= o.k; ++j) {
        const Scheme s = counted(j, j);
        all.pi.insert(all.pi.end(), s.pi.begin(), s.pi.end());
        all.l.insert(all.l.end(), s.l.begin(), s.l.end());
        all.u.insert(all.u.end(), s.u.begin(), s.u.end());
        all.counts.push_back(s.n);
    }
    return all;
}

// the stats block's lines after the times: the stages' counts summed over the shards, the devices
void printCounts(const SearchOptions& o, const std::vector<ShardResult>& shards, const std::vector<double>& load,
                 unsigned long long mapq30) {
    unsigned long long hits = 0, lociIn = 0, loci = 0, pairsIn = 0, pairsKept = 0, pairs = 0, bestIn = 0, bestKept = 0,
                       bestPairs = 0, unique = 0, links = 0, primaries = 0, anchors = 0, starts = 0, rescued = 0, capped = 0;
    for (const ShardResult& r : shards) {
        hits += r.hits;
        lociIn += r.loci.hits_in, loci += r.loci.loci;
        pairsIn += r.pairs.hits_in, pairsKept += r.pairs.kept, pairs += r.pairs.pairs;
        bestIn += r.best.hits_in, bestKept += r.best.kept, bestPairs += r.best.pairs, unique += r.best.unique_pairs;
        links += r.links.links, primaries += r.links.primaries;
        anchors += r.rescue.anchors, starts += r.rescue.starts, rescued += r.rescue.rescued, capped += r.rescue.capped_queries;
    }
    std::printf("  number of hits:      %10llu\n", hits);
    if (o.lociOn) std::printf("  loci:                %llu of %llu hits\n", loci, lociIn);
    if (o.paired) std::printf("  pairs:               %llu of %llu hits, %llu pairs\n", pairsKept, pairsIn, pairs);
    if (o.bestPairs)
        std::printf("  best pairs:          %llu of %llu hits, %llu pairs, %llu unique (delta %llu)\n", bestKept, bestIn,
                    bestPairs, unique, (unsigned long long)o.bestDelta);
    if (o.sam)
        std::printf("  pair links:          %llu links, %llu primary, %llu pairs with MAPQ >= 30\n", links, primaries, mapq30);
    if (o.rescue)
        std::printf("  rescue:              %llu mates from %llu anchors, %llu starts, %llu reads capped\n", rescued, anchors,
                    starts, capped);
    // ("ld index" above is the part of the load that the ingest did not hide; this is the whole load)
    std::printf("  index load:          %10.2fs (beside ld queries)\n", *std::max_element(load.begin(), load.end()));
    if (o.ngpu > 1)  // --gpus N: each device's index load and search (an imbalance shows by name)
        for (uint32_t g = 0; g < o.ngpu; ++g)
            std::printf("  device %u:            ld index %.2fs, search %.2fs, hits %llu\n", g, load[g], shards[g].search,
                        (unsigned long long)shards[g].hits);
}

}  // namespace

int cmdSearch(int argc, char** argv) {
    const SearchOptions o = parseSearchOptions(argc, argv);
    // sigma dispatch (search.cpp:276-291)
    const uint64_t sigma = readSigma(o.index);
    if (sigma != 5 && sigma != 6) throw CliError("unknown index with " + std::to_string(sigma) + " letters");
    Timing timing;
    StopWatch sw;

    // the index load, and beside it the queries
    IndexLoad L(o);
    L.start(o);
    const unsigned nt = hostThreads();
    const size_t per = o.reverse ? 2 : 1;  // patterns per read
    Queries Q;
    check(sahara_read_fasta(o.query.c_str(), (uint32_t)sigma, 2, nt, &Q.f), "reading queries");
    const size_t nq = verifyQueries(o, Q.f, per), nreads = (nq + per - 1) / per;  // reads that contribute a query
    timing.emplace_back("ld queries", sw.reset());
    std::printf(
        "config:\n"
        "  query:               %s\n"
        "  index:               %s\n"
        "  generator:           %s\n"
        "  dynamic expansion:   %s\n"
        "  allowed errors:      %d\n"
        "  reverse complements: %s\n"
        "  search mode:         %s\n"
        "  max hits:            %ld\n"
        "  output path:         %s\n"
        "fwd queries: %zu\nbwd queries: %zu\n",
        o.query.c_str(), o.index.c_str(), o.generator.c_str(), o.dynamic ? "true" : "false", o.k,
        o.reverse ? "true" : "false", o.besthits ? "besthits" : "all", o.maxHits, o.output.c_str(), nq / per, nq - nq / per);
    std::fflush(stdout);
    L.join();  // whatever of the load the ingest did not hide
    for (const std::string& e : L.errs)
        if (!e.empty()) throw CliError("loading index: " + e);
    for (void* c : L.ctx) configure(c, o);
    sahara_index_info info{};
    check(sahara_gpu_index_info(L.ctx[0], &info), "index info");
    timing.emplace_back("ld index", sw.reset());

    // the scheme: one expansion for queries[0].size(), the length all reads must have
    checkGenerator(o.generator);
    const uint64_t* offs = Q.f.offs;
    const uint32_t len = (uint32_t)(offs[1] - offs[0]);
    for (size_t r = 0; r < nreads; ++r)
        if (offs[r + 1] - offs[r] != len)
            throw CliError(fmtStr("query %zu has length %zu, but all queries must have the length of the first "
                                  "(%u): sahara expands one search scheme for queries[0].size()",
                                  per * r, (size_t)(offs[r + 1] - offs[r]), len));
    const Scheme scheme = searchedScheme(o, len, (int)sigma, (double)info.n);
    timing.emplace_back("searchScheme", sw.reset());

    // hits as compact records where they apply (no --max_hits, one index part, <= 15 errors;
    // SAHARA_CLI_FULL_HITS=1: whole records). --sam: always, for the record starts; its flags see to the first and
    // the last condition, and best pairs refuse a multi-part index
    const char* fullEnv = std::getenv("SAHARA_CLI_FULL_HITS");
    const bool compactOut = o.maxHits <= 0 && info.n_parts == 1 && o.k <= 15 && (o.sam || !(fullEnv && std::atoi(fullEnv)));
    if (o.sam && !compactOut) throw CliError("--sam needs a single-part index");

    // the reads sharded over the devices (a read and its reverse complement stay together; qids stay global)
    const PackedReads reads{Q.f.data, Q.f.n_count ? Q.f.n_pos : nullptr, Q.f.n_count};
    std::vector<ShardResult> shards(o.ngpu);
    {
        std::vector<std::thread> th;
        for (uint32_t g = 0; g < o.ngpu; ++g)
            th.emplace_back([&, g] {
                shards[g] = runShard(L.ctx[g], o, reads, len, (uint32_t)sigma, scheme, compactOut,
                                     queryShard(nq, per, o.ngpu, g, o.paired ? 2 : 1));
            });
        for (auto& t : th) t.join();
    }
    double loc = 0, aln = 0;
    for (const ShardResult& r : shards) {
        if (!r.err.empty()) throw CliError("search: " + r.err);
        loc = std::max(loc, r.locate), aln = std::max(aln, r.align);
    }
    timing.emplace_back("search", std::max(0.0, sw.reset() - loc - aln));
    timing.emplace_back("locate", loc);
    if (o.align) timing.emplace_back("align", aln);

    // the output; the hits are released once written
    unsigned long long mapq30 = 0;  // --sam: the pairs whose primary records carry a MAPQ of 30 or more
    {
        std::vector<HitPart> parts;
        for (ShardResult& r : shards) parts.push_back(std::move(r.part));
        if (o.sam) {
            for (const auto& hp : parts)
                for (const sahara_pair_link& l : hp.links) mapq30 += (l.flags & SAHARA_LINK_PRIMARY) && l.mapq >= 30;
            mapq30 /= 2;  // (two primary records per pair)
            writeSam(o.output, parts, SamReads{reads, len}, nq / 4, nt);
        } else {
            writeHits(o.output, parts, o.emitErrors, nt, o.emitCigar ? len : 0);
        }
    }
    if (o.pairSummary) {
        std::vector<PairSummaries> summaries;
        for (ShardResult& r : shards) summaries.push_back(std::move(r.summary));
        writePairSummary(*o.pairSummary, summaries);
    }
    timing.emplace_back("result", sw.reset());
    L.close();

    const double total = printTimings(timing);
    std::printf("  queries per second:  %10.0fq/s\n", (double)nq / total);
    printCounts(o, shards, L.seconds, mapq30);
    return 0;
}

}  // namespace sahara_cli
