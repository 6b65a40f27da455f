// main.cpp — the `sahara` command line, MI355X build.
//
// Drop-in for the reference CLI on the search hot path:
//   sahara index <fasta> [--ignore_unknown] [--dna4]          (src/sahara/index.cpp:20-121)
//   sahara search -q <fasta> -i <idx> [-o out] [-g gen] [-e k] [--no-reverse]
//                 [-m all|besthits] [-d ham|lev] [--max_hits n] [--limit_queries n]
//                                                            (src/sahara/search.cpp:22-291)
// Same flag spellings, defaults, stdout blocks, output format and exit codes
// (errors print their message and exit 1, main.cpp:13). Additions, all
// optional: --gpus N (query shards over N devices), --emit-errors (fourth
// output column e), --fm-only (reference execution: no text phase, LF-walk
// locate). The compute goes through the C ABI of libsahara_hip.so only.
// `search` is search.cpp.

#include <cstdlib>
#include <cstring>

#include "../csrc/fasta.h"
#include "options.h"

using namespace sahara_cli;
using namespace sahara_io;

namespace sahara_cli {
int cmdSearch(int argc, char** argv);  // search.cpp
}

namespace {

// ---------------------------------------------------------------- index ----

int cmdIndex(int argc, char** argv) {
    Opt ignore{{"--ignore_unknown"}, true}, dna4{{"--dna4"}, true}, gpu{{"--gpu"}, false, "0"};
    Parser p;
    for (Opt* o : {&ignore, &dna4, &gpu}) p.add(*o);
    p.parse(argc, argv, 2);
    if (p.positional.size() != 1) throw CliError("sahara index expects exactly one FASTA file");
    const std::string path = p.positional[0];
    const uint32_t sigma = dna4.given ? 5 : 6;

    std::printf("constructing an index for %s\n", path.c_str());
    Timing timing;
    StopWatch sw;

    // parallel whole-file ingest (fasta.h parseFastaParallel): records, ranks, first invalid character
    const unsigned nt = hostThreads();
    FastaData D = parseFastaParallel(path, sigma, nt);
    const uint64_t totalSize = D.ranks.size();
    if (ignore.given) {  // index.cpp:56-68: unknown characters become N (dna5) or a random base (dna4)
        if (dna4.given) {
            for (auto& v : D.ranks)
                if (v == 255 || v == 0 || v >= sigma) v = (uint8_t)(1 + std::rand() % 4);
        } else {
            parallelFor(nt, nt, [&](size_t t) {
                for (size_t i = D.ranks.size() * t / nt; i < D.ranks.size() * (t + 1) / nt; ++i)
                    if (D.ranks[i] == 255 || D.ranks[i] == 0 || D.ranks[i] >= sigma) D.ranks[i] = 4;
            });
        }
    } else if (D.bad) {
        const unsigned char ch = D.badChar;
        throw CliError(fmtStr("ref '%s' (%zu) has invalid character '%c' (0x%02x) at position %ld", D.badId.c_str(),
                              D.badRecord + 1, ch, ch, (long)D.badPos));
    }
    std::vector<uint64_t> lens(D.records());
    for (size_t r = 0; r < lens.size(); ++r) lens[r] = D.offs[r + 1] - D.offs[r];
    std::vector<uint8_t>& ranks = D.ranks;
    if (lens.empty()) throw CliError("reference file " + path + " was empty - abort\n");
    std::printf("config:\n  file: %s\n  sigma: %u\n  references: %zu\n  totalSize: %llu\n", path.c_str(), sigma, lens.size(),
                (unsigned long long)totalSize);
    timing.emplace_back("ld queries", sw.reset());

    void* ctx = nullptr;
    check(sahara_gpu_build((int)toU64(gpu.value, "--gpu"), ranks.data(), lens.data(), lens.size(), sigma, 16, &ctx),
          "index construction");
    timing.emplace_back("index creation", sw.reset());

    const std::string out = path + (dna4.given ? ".dna4.idx" : ".idx");
    check(sahara_gpu_save(ctx, out.c_str()), "saving index");
    sahara_gpu_close(ctx);
    timing.emplace_back("saving to disk", sw.reset());

    printTimings(timing);
    return 0;
}

// `sahara read_simulator` (src/sahara/read_simulator.cpp:13-82)
int cmdReadSimulator(int argc, char** argv) {
    Opt input{{"-i", "--input"}}, output{{"-o", "--output"}}, width{{"--fasta_line_length"}, false, "80"};
    Opt len{{"-l", "--read_length"}, false, "150"}, n{{"-n", "--number_of_reads"}, false, "1000"};
    Opt sub{{"--substitution_errors"}, false, "0"}, ins{{"--insertion_errors"}, false, "0"};
    Opt del{{"--deletion_errors"}, false, "0"}, err{{"-e", "--errors"}, false, "0"}, seed{{"--seed"}, false, "0"};
    Parser p;
    for (Opt* o : {&input, &output, &width, &len, &n, &sub, &ins, &del, &err, &seed}) p.add(*o);
    p.parse(argc, argv, 2);
    if (!p.positional.empty()) throw CliError("unexpected argument " + p.positional[0]);
    if (!output.given) throw CliError("option -o/--output is required");
    ReadSimulatorArgs a;
    a.haveInput = input.given;
    a.input = input.value;
    a.output = output.value;
    a.lineLength = toU64(width.value, "--fasta_line_length");
    a.readLength = toU64(len.value, "--read_length");
    a.nreads = toU64(n.value, "--number_of_reads");
    a.sub = toU64(sub.value, "--substitution_errors");
    a.ins = toU64(ins.value, "--insertion_errors");
    a.del = toU64(del.value, "--deletion_errors");
    a.errors = toU64(err.value, "--errors");
    a.seed = (uint32_t)toU64(seed.value, "--seed");
    return runReadSimulator(a);
}

void help() {
    std::printf(
        "sahara - readmapper (MI355X build)\n"
        "  sahara index <fasta> [--ignore_unknown] [--dna4] [--gpu N]\n"
        "  sahara search -q <fasta> -i <index> [-o <out>] [-g <generator>] [-e <k>] [--no-reverse]\n"
        "                [-m all|besthits] [-d ham|lev] [--max_hits <n>] [--limit_queries <n>]\n"
        "                [--gpus <N>] [--emit-errors] [--emit-cigar] [--fm-only]\n"
        "                [--loci] [--loci-window <n>]   one hit per locus (window: -e's value, or n)\n"
        "                [--paired] [--min-fragment <n>] [--max-fragment <n>]   the query file holds mate pairs\n"
        "                interleaved; only hits with a concordant mate are written (fragment 0..500, or n)\n"
        "                [--rescue <n>] [--rescue-anchors <a>]   with --paired: a hit without a mate gets its\n"
        "                fragment window scanned for the other read with up to n errors (1..8); a read with\n"
        "                more than a such hits is left alone (64; 0: no cap)\n"
        "                [--best-pairs] [--pair-delta <d>] [--pair-summary <file>]   with --paired: of a pair's\n"
        "                concordant placements only those within d errors (0; at most 30) of its best, each\n"
        "                position once; the file gets pair, best, next, n_fwd, n_rev per pair that keeps a hit\n"
        "                [--sam]   with --paired --best-pairs: -o becomes a SAM file, a record per kept hit with\n"
        "                its mate, MAPQ and CIGAR; a pair that keeps nothing writes its reads unmapped\n"
        "  sahara read_simulator -o <fasta> [-i <reference>] [-l <len>] [-n <reads>] [-e <errors>]\n"
        "                [--substitution_errors n] [--insertion_errors n] [--deletion_errors n]\n"
        "                [--fasta_line_length n] [--seed s]\n"
        "  sahara search_scheme list-generators\n");
}

}  // namespace

int main(int argc, char** argv) {
    // six streams per device context: their own hardware queues (HIP's default
    // is 4 per process), set before the first HIP call
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    try {
        if (argc < 2 || !std::strcmp(argv[1], "--help") || !std::strcmp(argv[1], "-h")) {
            help();
            return argc < 2 ? 1 : 0;
        }
        const std::string cmd = argv[1];
        if (cmd == "index") return cmdIndex(argc, argv);
        if (cmd == "search") return cmdSearch(argc, argv);
        if (cmd == "read_simulator") return cmdReadSimulator(argc, argv);
        if (cmd == "search_scheme" && argc >= 3 && std::string(argv[2]) == "list-generators") {
            const char* names[64];
            const char* descs[64];
            int n = sahara_scheme_generators(names, descs, 64);
            for (int i = 0; i < n; ++i) std::printf("%15s - %s\n", names[i], descs[i]);
            return 0;
        }
        throw CliError("unknown command " + cmd);
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
