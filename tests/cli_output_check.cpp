// cli_output_check.cpp — the command line's writers (sahara_amd/cli/output.h)
// without a device: tests/test_cli_output.py writes a planted case to a file
// (kept rows, links, alignments, packed reads, record starts); this program
// forms the shards' HitParts from it in several layouts and lets writeSam and
// writeHits write each, with small blocks and 1 and 3 threads. The wrapper
// compares the files byte for byte with its models. Links libsahara_hip.so
// for sahara_cigar and the records' release; makes no HIP call.
//
//   cli_output_check <case file> <output directory>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sahara_amd/cli/output.h"

using namespace sahara_cli;

namespace {

struct Case {
    uint64_t nHits = 0, nPairs = 0, len = 0, nRecords = 0;
    std::vector<uint64_t> cuts;  // the layouts' shard borders, as pairs, each list ended by nPairs
    std::vector<uint64_t> starts;
    std::vector<sahara_hit> rows;  // the call's qids
    std::vector<sahara_pair_link> links;
    std::vector<sahara_alignment> aln;
    std::vector<uint8_t> codes;
    std::vector<uint64_t> npos;
};

template <typename T>
std::vector<T> take(std::ifstream& f, uint64_t n) {
    std::vector<T> v(n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    if (!f) throw std::runtime_error("case file too short");
    return v;
}

Case readCase(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open case file");
    const std::vector<uint64_t> h = take<uint64_t>(f, 7);
    Case c;
    c.nHits = h[0], c.nPairs = h[1], c.len = h[2], c.nRecords = h[3];
    c.cuts = take<uint64_t>(f, h[6]);
    c.starts = take<uint64_t>(f, c.nRecords + 1);
    c.rows = take<sahara_hit>(f, c.nHits);
    c.links = take<sahara_pair_link>(f, c.nHits);
    c.aln = take<sahara_alignment>(f, c.nHits);
    c.codes = take<uint8_t>(f, h[4]);
    c.npos = take<uint64_t>(f, h[5]);
    return c;
}

template <typename T>
T* cArray(const std::vector<T>& v) {  // malloc'ed, as the library hands its arrays over
    T* p = static_cast<T*>(std::malloc(std::max<size_t>(1, v.size() * sizeof(T))));
    if (!p) throw std::bad_alloc();
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// The shard of pairs [pa, pb): its hits with local qids. compact: the records in blocks of `width` queries,
// of which some hold no hit, and one more, empty, at the end.
HitPart shardOf(const Case& c, uint64_t pa, uint64_t pb, bool compact, uint64_t width) {
    HitPart P;
    P.qidOffset = 4 * pa;
    std::vector<sahara_hit> mine;
    for (uint64_t k = 0; k < c.nHits; ++k)
        if (c.rows[k].qid >= 4 * pa && c.rows[k].qid < 4 * pb) {
            sahara_hit h = c.rows[k];
            h.qid -= P.qidOffset;
            mine.push_back(h);
            P.links.push_back(c.links[k]);
            P.aln.push_back(c.aln[k]);
        }
    P.n = mine.size();
    if (!compact) {
        P.hits = cArray(mine);
        return P;
    }
    std::vector<uint64_t> recs, end, qid0;
    size_t k = 0;
    for (uint64_t q = 0; q < 4 * (pb - pa) + width; q += width) {  // (the last round: the empty block)
        for (; k < mine.size() && mine[k].qid < q + width; ++k)
            recs.push_back((mine[k].qid - q) << 36 | (c.starts[mine[k].seq_id] + mine[k].pos) << 4 | mine[k].err);
        qid0.push_back(q);
        end.push_back(k);
    }
    P.compact = true;
    P.blocks.recs = cArray(recs);
    P.blocks.n_hits = recs.size();
    P.blocks.block_qid0 = cArray(qid0);
    P.blocks.block_end = cArray(end);
    P.blocks.n_blocks = end.size();
    P.blocks.rec_starts = c.starts.data();
    P.blocks.n_records = c.nRecords;
    return P;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        const Case c = readCase(argv[1]);
        const std::string dir = argv[2];
        const SamReads R{{c.codes.data(), c.npos.empty() ? nullptr : c.npos.data(), c.npos.size()}, (uint32_t)c.len};
        int layout = 0;
        for (size_t i = 0; i < c.cuts.size(); ++layout) {
            std::vector<HitPart> compact, whole;
            for (uint64_t pa = 0;; pa = c.cuts[i++]) {
                compact.push_back(shardOf(c, pa, c.cuts[i], true, 6));
                whole.push_back(shardOf(c, pa, c.cuts[i], false, 0));
                if (c.cuts[i] == c.nPairs) break;
            }
            ++i;
            for (unsigned nt : {1u, 3u}) {
                const std::string tag = "_L" + std::to_string(layout) + "_t" + std::to_string(nt);
                writeSam(dir + "/sam" + tag, compact, R, c.nPairs, nt, 3);
                writeHits(dir + "/plain" + tag, compact, false, nt, 0, 5);
                writeHits(dir + "/errors" + tag, compact, true, nt, 0, 5);
                writeHits(dir + "/cigar" + tag, compact, true, nt, (uint32_t)c.len, 5);
                writeHits(dir + "/whole" + tag, whole, true, nt, (uint32_t)c.len, 5);
            }
        }
        std::printf("%d layouts\n", layout);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
