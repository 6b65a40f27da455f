// options.h — what the commands share (errors, the option parser, the stats block's times), `read_simulator`'s
// arguments, and the options of `sahara search` as typed values, checked as far as the command line alone allows.
#pragma once
#include <algorithm>
#include <cctype>
#include <charconv>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/sahara_hip.h"

namespace sahara_cli {

struct CliError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

__attribute__((format(printf, 1, 2))) inline std::string fmtStr(const char* f, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

inline void check(int rc, const char* what) {
    if (rc != 0) throw CliError(std::string(what) + ": " + sahara_gpu_last_error());
}

struct Opt {
    std::vector<std::string> names;
    bool flag;
    std::string value;
    bool given = false;
    Opt(std::vector<std::string> n, bool f = false, std::string v = {}) : names(std::move(n)), flag(f), value(std::move(v)) {}
};

struct Parser {
    std::map<std::string, Opt*> byName;
    std::vector<std::string> positional;
    void add(Opt& o) {
        for (auto& n : o.names) byName[n] = &o;
    }
    void parse(int argc, char** argv, int first) {
        for (int i = first; i < argc; ++i) {
            std::string a = argv[i];
            std::string val;
            bool hasVal = false;
            if (a.size() > 2 && a[0] == '-' && a.find('=') != std::string::npos) {
                val = a.substr(a.find('=') + 1);
                a = a.substr(0, a.find('='));
                hasVal = true;
            }
            auto it = byName.find(a);
            if (it == byName.end()) {
                if (!a.empty() && a[0] == '-' && a.size() > 1 && !std::isdigit((unsigned char)a[1]))
                    throw CliError("unknown option " + a);
                positional.push_back(a);
                continue;
            }
            Opt& o = *it->second;
            o.given = true;
            if (o.flag) continue;
            if (!hasVal) {
                if (i + 1 >= argc) throw CliError("option " + a + " expects a value");
                val = argv[++i];
            }
            o.value = val;
        }
    }
};

inline uint64_t toU64(const std::string& s, const char* what) {
    uint64_t v = 0;
    auto r = std::from_chars(s.data(), s.data() + s.size(), v);
    if (r.ec != std::errc() || r.ptr != s.data() + s.size()) throw CliError(std::string("invalid value for ") + what + ": " + s);
    return v;
}

// utils/StopWatch.h:8-28
struct StopWatch {
    std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now();
    double peek() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count(); }
    double reset() {
        const double d = peek();
        start = std::chrono::steady_clock::now();
        return d;
    }
};

// the "stats:" block's steps and their total, which it returns
using Timing = std::vector<std::tuple<std::string, double>>;
inline double printTimings(const Timing& timing) {
    std::printf("stats:\n");
    double total = 0;
    for (auto& [key, t] : timing) {
        std::printf("  %-20s %10.2fs\n", (key + " time:").c_str(), t);
        total += t;
    }
    std::printf("  total time:          %10.2fs\n", total);
    return total;
}

struct ReadSimulatorArgs {
    std::string input, output;
    size_t lineLength = 80, readLength = 150, nreads = 1000, sub = 0, ins = 0, del = 0, errors = 0;
    uint32_t seed = 0;
    bool haveInput = false;
};
int runReadSimulator(const ReadSimulatorArgs& a);  // read_simulator.cpp

// What each group of flags means: the help text (main.cpp) and docs/semantics.md.
struct SearchOptions {
    std::string query, index, output, generator;
    bool dynamic = false, reverse = true, besthits = false, edit = true, emitErrors = false, emitCigar = false;
    bool fmOnly = false, lociOn = false, paired = false, rescue = false, bestPairs = false, sam = false;
    bool align = false;  // --emit-cigar or --sam: the alignment call
    int k = 0;
    long maxHits = 0;
    uint32_t ngpu = 1, alignK = 0;  // alignK: the alignment's bound, the larger of -e and --rescue
    uint64_t lociW = 0, fragLo = 0, fragHi = 0, rescueK = 0, rescueA = 0, bestDelta = 0;
    uint64_t limit = UINT64_MAX;  // --limit_queries (not given: no cut)
    // a bad --limit_queries without --paired is refused only once the index is read, as it always was
    std::string limitError;
    std::optional<std::string> pairSummary;  // --pair-summary's file
};

// argv[2..] of `sahara search`; throws the refusals that need neither the queries nor the index
inline SearchOptions parseSearchOptions(int argc, char** argv) {
    Opt query{{"-q", "--query"}}, index{{"-i", "--index"}}, output{{"-o", "--output"}, false, "sahara-output.txt"};
    Opt gen{{"-g", "--generator"}, false, "h2-k2"}, dyn{{"--dynamic_generator"}, true};
    Opt errors{{"-e", "--errors"}, false, "0"}, noRev{{"--no-reverse"}, true};
    Opt mode{{"-m", "--search_mode"}, false, "all"}, dist{{"-d", "--distance-metric"}, false, "lev"};
    Opt maxHits{{"--max_hits"}, false, "0"}, limit{{"--limit_queries"}};
    Opt gpus{{"--gpus"}, false, "1"}, emitErr{{"--emit-errors"}, true}, fmOnly{{"--fm-only"}, true};
    Opt emitCigar{{"--emit-cigar"}, true}, loci{{"--loci"}, true}, lociWindow{{"--loci-window"}};
    Opt paired{{"--paired"}, true}, minFrag{{"--min-fragment"}, false, "0"}, maxFrag{{"--max-fragment"}, false, "500"};
    Opt rescue{{"--rescue"}}, rescueAnchors{{"--rescue-anchors"}, false, "64"};
    Opt bestPairs{{"--best-pairs"}, true}, pairDelta{{"--pair-delta"}, false, "0"}, pairSummary{{"--pair-summary"}};
    Opt sam{{"--sam"}, true};
    Parser p;
    for (Opt* o : {&query, &index, &output, &gen, &dyn, &errors, &noRev, &mode, &dist, &maxHits, &limit, &gpus,
                   &emitErr, &fmOnly, &emitCigar, &loci, &lociWindow, &paired, &minFrag, &maxFrag, &rescue, &rescueAnchors,
                   &bestPairs, &pairDelta, &pairSummary, &sam})
        p.add(*o);
    p.parse(argc, argv, 2);
    if (!p.positional.empty()) throw CliError("unexpected argument " + p.positional[0]);
    if (!query.given) throw CliError("option -q/--query is required");
    if (!index.given) throw CliError("option -i/--index is required");
    if (mode.value != "all" && mode.value != "besthits") throw CliError("invalid value for --search_mode: " + mode.value);
    if (dist.value != "ham" && dist.value != "lev") throw CliError("invalid value for --distance-metric: " + dist.value);
    SearchOptions o;
    o.query = query.value;
    o.index = index.value;
    o.output = output.value;
    o.generator = gen.value;
    o.dynamic = dyn.given;
    o.reverse = !noRev.given;
    o.emitErrors = emitErr.given;
    o.fmOnly = fmOnly.given;
    o.besthits = mode.value == "besthits";
    o.edit = dist.value == "lev";
    o.k = (int)toU64(errors.value, "--errors");
    o.maxHits = std::strtol(maxHits.value.c_str(), nullptr, 10);
    o.ngpu = (uint32_t)std::max<uint64_t>(1, toU64(gpus.value, "--gpus"));
    o.lociOn = loci.given || lociWindow.given;
    o.lociW = lociWindow.given ? toU64(lociWindow.value, "--loci-window") : (uint64_t)o.k;
    if (o.lociOn && o.lociW > 0xFFFFFFFFull) throw CliError("--loci-window is at most 4294967295");
    o.fragLo = toU64(minFrag.value, "--min-fragment");
    o.fragHi = toU64(maxFrag.value, "--max-fragment");
    o.paired = paired.given;
    if ((minFrag.given || maxFrag.given) && !o.paired) throw CliError("--min-fragment / --max-fragment need --paired");
    try {
        if (limit.given) o.limit = toU64(limit.value, "--limit_queries");
    } catch (const CliError& e) {
        o.limitError = e.what();
    }
    if (o.paired) {
        if (!o.reverse) throw CliError("--paired needs the reverse complements: it cannot go with --no-reverse");
        if (o.fragLo > o.fragHi) throw CliError("--min-fragment is above --max-fragment");
        if (o.fragHi > 0xFFFFFFFFull) throw CliError("--max-fragment is at most 4294967295");
        if (!o.limitError.empty()) throw CliError(o.limitError);
        if (limit.given && o.limit % 4)
            throw CliError("--paired: --limit_queries must be a multiple of 4 (a pair is two mates and their reverse "
                           "complements)");
    }
    o.bestPairs = bestPairs.given;
    o.sam = sam.given;
    if (o.sam) {
        if (!o.paired || !o.bestPairs)
            throw CliError("--sam needs --paired --best-pairs (a SAM record names its mate, and a pair's primary "
                           "placement and MAPQ come from the best-pairs rule)");
        if (o.maxHits > 0) throw CliError("--sam cannot go with --max_hits (the cut would drop linked hits)");
    }
    o.emitCigar = emitCigar.given;
    o.align = o.emitCigar || o.sam;  // --sam implies the alignment call of --emit-cigar
    if (o.align && o.k > SAHARA_ALIGN_MAX_ERR)
        throw CliError(std::string(o.sam ? "--sam" : "--emit-cigar") + " aligns at most " +
                       std::to_string(SAHARA_ALIGN_MAX_ERR) + " errors (-e)");
    o.rescue = rescue.given;
    if (rescueAnchors.given && !o.rescue) throw CliError("--rescue-anchors needs --rescue");
    o.rescueK = o.rescue ? toU64(rescue.value, "--rescue") : 0;
    o.rescueA = toU64(rescueAnchors.value, "--rescue-anchors");
    if (o.rescue) {
        if (!o.paired) throw CliError("--rescue needs --paired (a mate is looked for in the fragment window)");
        if (o.rescueK < 1 || o.rescueK > SAHARA_ALIGN_MAX_ERR)
            throw CliError("--rescue takes 1 to " + std::to_string(SAHARA_ALIGN_MAX_ERR) + " errors");
        if (o.rescueA > 0xFFFFFFFFull) throw CliError("--rescue-anchors is at most 4294967295");
    }
    if ((pairDelta.given || pairSummary.given) && !o.bestPairs)
        throw CliError("--pair-delta / --pair-summary need --best-pairs");
    if (o.bestPairs && !o.paired) throw CliError("--best-pairs needs --paired (the placements ranked are pairs')");
    if (pairSummary.given) o.pairSummary = pairSummary.value;
    o.bestDelta = toU64(pairDelta.value, "--pair-delta");
    if (o.bestDelta > SAHARA_BEST_PAIRS_MAX_DELTA)
        throw CliError("--pair-delta is at most " + std::to_string(SAHARA_BEST_PAIRS_MAX_DELTA));
    o.alignK = (uint32_t)std::max<uint64_t>((uint64_t)o.k, o.rescueK);
    return o;
}

}  // namespace sahara_cli
