// capi_ctx.cpp — context lifecycle and the index calls of the C ABI
// (include/sahara_hip.h): NUMA placement, build, open, info, export, save.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"
#include "idx_format.h"
#include "pair_links_core.h"

using namespace sahara;

namespace sahara {

thread_local std::string g_err;

// SAHARA_DEVICE_MAP=a,b,c (test hook): context device d opens HIP device
// list[d], so that `sahara search --gpus N` and concurrent contexts run their
// multi-device code path on one GPU (tests/test_multi_device.py)
static int mapDevice(int device) {
    const char* e = std::getenv("SAHARA_DEVICE_MAP");
    if (!e || !*e) return device;
    std::vector<int> map;
    for (const char* p = e; *p;) {
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p) throw Error(std::string("SAHARA_DEVICE_MAP: not a list of device numbers: ") + e);
        map.push_back((int)v);
        p = *end == ',' ? end + 1 : end;
        if (*end && *end != ',') throw Error(std::string("SAHARA_DEVICE_MAP: not a list of device numbers: ") + e);
    }
    if (device < 0 || (size_t)device >= map.size())
        throw Error("SAHARA_DEVICE_MAP has no entry for device " + std::to_string(device));
    return map[(size_t)device];
}

// The CPUs of NUMA node `node` that this process may run on.
Placement placementOfNode(int node) {
    Placement pl;
    pl.node = node;
    if (node < 0) return pl;
    std::FILE* f = std::fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r");
    if (!f) return pl;
    char buf[8192] = {0};
    const size_t got = std::fread(buf, 1, sizeof(buf) - 1, f);
    std::fclose(f);
    buf[got] = 0;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return pl;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (const char* p = buf; *p && *p != '\n';) {  // "0-15,64-79"
        char* end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') b = std::strtol(end + 1, &end, 10);
        for (long i = a; i <= b && i < CPU_SETSIZE; ++i)
            if (CPU_ISSET(i, &allowed)) CPU_SET(i, &set);
        p = *end == ',' ? end + 1 : end;
    }
    pl.cpus = set;
    pl.ncpus = CPU_COUNT(&set);
    return pl;
}

// The CPUs of the device's NUMA node that this process may run on (Placement).
static void placeNear(Ctx* c) {
    const char* e = std::getenv("SAHARA_NUMA");
    if (e && std::atoi(e) == 0) return;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), c->device) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    std::string id(bdf);
    for (char& ch : id) ch = (char)std::tolower((unsigned char)ch);
    int node = -1;
    if (std::FILE* f = std::fopen(("/sys/bus/pci/devices/" + id + "/numa_node").c_str(), "r")) {
        if (std::fscanf(f, "%d", &node) != 1) node = -1;
        std::fclose(f);
    }
    c->place = placementOfNode(node);
}

// host threads a context uses for one job: its node's allowed CPUs (or the
// process's), at most cap
unsigned hostThreads(const Ctx* c, unsigned cap) {
    unsigned n = (unsigned)c->place.ncpus;
    if (n == 0) {
        cpu_set_t s;
        CPU_ZERO(&s);
        n = sched_getaffinity(0, sizeof(s), &s) == 0 ? (unsigned)CPU_COUNT(&s) : std::thread::hardware_concurrency();
    }
    return std::max(1u, std::min(cap, n));
}

Ctx* newCtx(int device) {
    int n = 0;
    SH_HIP(hipGetDeviceCount(&n));
    const int hipDev = mapDevice(device);
    if (hipDev < 0 || hipDev >= n)
        throw Error("no HIP device " + std::to_string(hipDev) + " (found " + std::to_string(n) + ")");
    SH_HIP(hipSetDevice(hipDev));
    auto c = std::make_unique<Ctx>();
    c->device = hipDev;
    placeNear(c.get());
    hipDeviceProp_t prop;
    SH_HIP(hipGetDeviceProperties(&prop, hipDev));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        throw Error(std::string("libsahara_hip is built for gfx950 (MI355X); device is ") + prop.gcnArchName);
    c->numCU = prop.multiProcessorCount;
    // (No stream gets a CU mask: with a CU-masked stream in the process the
    // memory-bound kernels on the other streams ran 1.4-1.8x longer, r5.)
    for (Stream* s : {&c->st, &c->stB, &c->stC, &c->stD, &c->stE, &c->stF}) *s = Stream(hipStreamNonBlocking);
    for (Event* e : {&c->outCopied[0], &c->outCopied[1], &c->locStart, &c->locDone, &c->sortDone, &c->totalsDown,
                     &c->flagsDown, &c->recsMade})
        *e = Event(hipEventDefault);
    for (Event* stage : {c->stageStart, c->stageDone})
        for (uint32_t s = 0; s < kStages; ++s) stage[s] = Event(hipEventDefault);
    for (Event* e : {&c->totalsDownSleep, &c->flagsDownSleep}) *e = Event(hipEventDisableTiming | hipEventBlockingSync);
    for (auto& e : c->ringEv) e = Event(hipEventDisableTiming);
    // the streamed upload's pinned ring, pinned while the caller builds or
    // loads the index (pinning 256 MB takes ~50 ms)
    Ctx* raw = c.get();
    raw->ringInit = std::thread([raw] {
        raw->place.bind();  // pinned pages first touched on the device's node
        (void)hipSetDevice(raw->device);
        try {
            raw->ring.reserve(Ctx::kRingSlots * Ctx::kRingSlot, hipHostMallocPortable);
        } catch (const Error&) {
            raw->ringFailed = true;
        }
        try {
            raw->downRing.reserve(Ctx::kDownSlots * Ctx::kDownSlot / sizeof(uint64_t), hipHostMallocPortable);
        } catch (const Error&) {  // no compact download: hits go to a pinned sink whole
        }
    });
    for (auto& sl : c->slot) {
        for (Event* e : {&sl.fmStart, &sl.seedDone, &sl.seedDone0, &sl.seedMid, &sl.fmBegin, &sl.fmDone, &sl.textStart,
                         &sl.textDone, &sl.free, &sl.textMid0, &sl.textMid1})
            *e = Event(hipEventDefault);
        sl.small.reserve(kSlotWords);
        sl.queues.reserve(kQueuesWords);
    }
    for (auto& p : c->outStage) p.reserve(Ctx::kOutChunk);
    c->small.reserve(8);
    c->counters.reserve(kCounters);
    SH_HIP(hipMemset(c->counters.ptr, 0, kCounters * sizeof(unsigned long long)));
    return c.release();
}

Ctx* ctxOf(void* p) {
    if (!p) throw Error("null context");
    Ctx* c = static_cast<Ctx*>(p);
    SH_HIP(hipSetDevice(c->device));
    return c;
}

// an .idx image (one part or several) -> a context holding every part
Ctx* openImage(int device, const uint8_t* buf, size_t bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&t0] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const std::vector<IdxParts> parts = parseIdxAll(buf, bytes);
    const double tParse = since();
    std::unique_ptr<Ctx> c(newCtx(device));
    const double tCtx = since();
    if (std::getenv("SAHARA_TIMING"))  // (the parts' own steps follow from buildFromParts)
        std::fprintf(stderr, "[sahara] open: parse %.1f ms, context %.1f ms\n", tParse, tCtx - tParse);
    uint64_t rec0 = 0, nmax = 0;
    c->partRec0.clear();
    // the image's arrays through the pinned ring (SAHARA_LOAD_RING=0: pageable copies)
    Ctx* raw = c.get();
    const HostUpload viaRing = [raw](void* dst, const void* src, size_t n, hipStream_t s) {
        uploadViaRing(raw, dst, src, n, s);
    };
    const char* lr = std::getenv("SAHARA_LOAD_RING");
    const HostUpload* up = lr && std::atoi(lr) == 0 ? nullptr : &viaRing;
    for (size_t p = 0; p < parts.size(); ++p) {
        const IdxParts& P = parts[p];
        if (p) c->more.emplace_back();
        buildFromParts(partOf(c.get(), (uint32_t)p), P.sigma, P.n, P.recLens.data(), P.recLens.size(), P.rate, P.bwtF,
                       P.bwtR, P.sampled, P.samples, P.nsamples, c->st, parts.size() == 1, up);
        c->partRec0.push_back(rec0);
        rec0 += P.recLens.size();
        nmax = std::max(nmax, P.n);
    }
    if (parts.size() > 1) {
        const uint32_t K = kmerDepth(nmax, (uint32_t)parts.size());
        for (uint32_t p = 0; p < parts.size(); ++p) buildKmerTable(partOf(c.get(), p), K, c->st);
    }
    return c.release();
}

}  // namespace sahara

extern "C" {

const char* sahara_gpu_last_error(void) { return g_err.c_str(); }

const char* sahara_build_id(void) { return SAHARA_BUILD_ID; }

int sahara_gpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sahara_gpu_build(int device, const uint8_t* ranks, const uint64_t* rec_lens, uint64_t n_records, uint32_t sigma,
                     uint32_t sampling_rate, void** ctx) {
    return guarded([&] {
        std::unique_ptr<Ctx> c(newCtx(device));
        const std::vector<uint64_t> first = splitRecords(rec_lens, n_records);
        if (first.size() == 2) {
            buildFromText(c->I, ranks, rec_lens, n_records, sigma, sampling_rate, c->st);
        } else {  // parts at record boundaries, then their k-mer tables at one common depth
            uint64_t off = 0, nmax = 0;
            for (size_t p = 0; p + 1 < first.size(); ++p) {
                uint64_t syms = 0, n = 0;
                for (uint64_t r = first[p]; r < first[p + 1]; ++r) syms += rec_lens[r];
                n = syms + (first[p + 1] - first[p]);
                nmax = std::max(nmax, n);
                if (p) c->more.emplace_back();
                buildFromText(partOf(c.get(), (uint32_t)p), ranks + off, rec_lens + first[p], first[p + 1] - first[p],
                              sigma, sampling_rate, c->st, false);
                off += syms;
            }
            c->partRec0.assign(first.begin(), first.end() - 1);
            const uint32_t K = kmerDepth(nmax, (uint32_t)first.size() - 1);
            for (uint32_t p = 0; p + 1 < first.size(); ++p) buildKmerTable(partOf(c.get(), p), K, c->st);
        }
        *ctx = c.release();
    });
}

int sahara_gpu_open(int device, const void* idx_image, size_t idx_bytes, void** ctx) {
    return guarded([&] { *ctx = openImage(device, static_cast<const uint8_t*>(idx_image), idx_bytes); });
}

int sahara_gpu_open_file(int device, const char* path, void** ctx) {
    return guarded([&] {
        const std::vector<uint8_t> buf = readFile(path);
        *ctx = openImage(device, buf.data(), buf.size());
    });
}

int sahara_gpu_index_info(void* ctx, sahara_index_info* info) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        info->sigma = c->I.sigma;
        info->sampling_rate = c->I.rate;
        info->n = info->n_records = info->n_samples = info->device_bytes = 0;
        for (uint32_t p = 0; p <= c->more.size(); ++p) {  // totals over the parts
            const DeviceIndex& D = partOf(c, p);
            info->n += D.n;
            info->n_records += D.recLens.size();
            info->n_samples += D.nsamples;
            info->device_bytes += D.deviceBytes();
        }
        info->n_parts = (uint32_t)c->more.size() + 1;
        info->kmer_depth = c->I.kmerK;
    });
}

int sahara_gpu_export(void* ctx, uint8_t* bwt_f, uint8_t* bwt_r, uint64_t* sampled_bits, uint32_t* samples,
                      uint64_t* C, uint64_t* rec_lens) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        DeviceIndex& D = partOf(c, c->exportPart);
        exportParts(D, bwt_f, bwt_r, sampled_bits, samples, c->st);
        if (C) std::memcpy(C, D.C, (D.sigma + 1) * 8);
        if (rec_lens) std::memcpy(rec_lens, D.recLens.data(), D.recLens.size() * 8);
    });
}

int sahara_gpu_export_sa(void* ctx, uint32_t* sa) {
    return guarded([&] {
        const DeviceIndex& D = partOf(ctxOf(ctx), ctxOf(ctx)->exportPart);
        SH_HIP(hipMemcpy(sa, D.saFull.ptr, D.n * 4, hipMemcpyDeviceToHost));
    });
}

int sahara_gpu_export_text(void* ctx, uint8_t* text) {
    return guarded([&] {
        const DeviceIndex& D = partOf(ctxOf(ctx), ctxOf(ctx)->exportPart);
        std::vector<uint32_t> t3(((D.n + 31) / 32) * 4);
        SH_HIP(hipMemcpy(t3.data(), D.text3.ptr, t3.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < D.n; ++i) {
            const uint32_t* b = &t3[(i / 32) * 4];
            const uint32_t j = (uint32_t)(i & 31);
            text[i] = (uint8_t)(((b[0] >> j) & 1u) | (((b[1] >> j) & 1u) << 1) | (((b[2] >> j) & 1u) << 2));
        }
    });
}

int sahara_gpu_part_info(void* ctx, uint32_t part, sahara_index_info* info) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (part > c->more.size()) throw Error("no index part " + std::to_string(part));
        const DeviceIndex& D = partOf(c, part);
        info->sigma = D.sigma;
        info->sampling_rate = D.rate;
        info->n = D.n;
        info->n_records = D.recLens.size();
        info->n_samples = D.nsamples;
        info->device_bytes = D.deviceBytes();
        info->n_parts = (uint32_t)c->more.size() + 1;
        info->kmer_depth = D.kmerK;
    });
}

int sahara_gpu_select_part(void* ctx, uint32_t part) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (part > c->more.size()) throw Error("no index part " + std::to_string(part));
        c->exportPart = part;
    });
}

int sahara_gpu_set_mode(void* ctx, int verify, int locate_sa) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        c->verify = verify != 0;
        c->locateSA = locate_sa != 0;
    });
}

int sahara_gpu_set_loci(void* ctx, int on, uint32_t window) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        c->loci.on = on != 0;
        c->loci.window = on ? window : 0u;
    });
}

int sahara_gpu_loci_stats(void* ctx, sahara_loci_stats* stats) {
    return guarded([&] {
        if (!stats) throw Error("sahara_gpu_loci_stats: null output");
        *stats = ctxOf(ctx)->stageStats.loci;
    });
}

int sahara_gpu_set_pairs(void* ctx, int on, uint32_t min_fragment, uint32_t max_fragment) {
    return guarded([&] {
        if (on && min_fragment > max_fragment) throw Error("sahara_gpu_set_pairs: min_fragment is above max_fragment");
        Ctx* c = ctxOf(ctx);
        c->pairs.on = on != 0;
        c->pairs.minFrag = on ? min_fragment : 0u;
        c->pairs.maxFrag = on ? max_fragment : 0u;
    });
}

int sahara_gpu_pairs_stats(void* ctx, sahara_pairs_stats* stats) {
    return guarded([&] {
        if (!stats) throw Error("sahara_gpu_pairs_stats: null output");
        *stats = ctxOf(ctx)->stageStats.pairs;
    });
}

int sahara_gpu_set_best_pairs(void* ctx, int on, uint32_t delta) {
    return guarded([&] {
        if (on && delta > SAHARA_BEST_PAIRS_MAX_DELTA)
            throw Error("sahara_gpu_set_best_pairs: delta must be in [0, " + std::to_string(SAHARA_BEST_PAIRS_MAX_DELTA) +
                        "]");
        Ctx* c = ctxOf(ctx);
        c->pairs.best = on != 0;
        c->pairs.delta = on ? delta : 0u;
    });
}

int sahara_gpu_pair_summary(void* ctx, sahara_pair_summary* out, uint64_t capacity, uint64_t* n_pairs) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!c->pairs.summaryOn) throw Error("sahara_gpu_pair_summary: the last search call ran without best pairs");
        if (n_pairs) *n_pairs = c->pairs.summaryPairs;
        if (!out && capacity == 0) return;  // the count alone
        if (capacity < c->pairs.summaryPairs) throw Error("sahara_gpu_pair_summary: capacity too small");
        if (c->pairs.summaryPairs && !out) throw Error("sahara_gpu_pair_summary: null output");
        std::copy_n(c->pairs.summary.ptr, c->pairs.summaryPairs, out);
    });
}

// (the pairs are counted from the summary, so an overflow re-run leaves the figures of the batches that count)
int sahara_gpu_best_pairs_stats(void* ctx, sahara_best_pairs_stats* stats) {
    return guarded([&] {
        if (!stats) throw Error("sahara_gpu_best_pairs_stats: null output");
        const Ctx* c = ctxOf(ctx);
        sahara_best_pairs_stats s{};
        if (c->pairs.summaryOn) {
            const sahara_pairs_stats& p = c->stageStats.pairs;
            s.hits_in = p.hits_in;
            s.kept = p.kept;
            s.batches = p.batches;
            s.kernel_ms = p.kernel_ms;
            for (uint64_t i = 0; i < c->pairs.summaryPairs; ++i) {
                const sahara_pair_summary& x = c->pairs.summary.ptr[i];
                s.pairs += x.best != 255;
                s.unique_pairs += x.n_fwd == 1 && x.n_rev == 1;
            }
        }
        *stats = s;
    });
}

int sahara_gpu_set_pair_links(void* ctx, int on) {
    return guarded([&] { ctxOf(ctx)->pairs.links = on != 0; });
}

int sahara_gpu_pair_links(void* ctx, sahara_pair_link* out, uint64_t capacity, uint64_t* n_links) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!c->pairs.linksOn) throw Error("sahara_gpu_pair_links: the last search call ran without pair links");
        if (n_links) *n_links = c->pairs.linkCount;
        if (!out && capacity == 0) return;  // the count alone
        if (capacity < c->pairs.linkCount) throw Error("sahara_gpu_pair_links: capacity too small");
        if (c->pairs.linkCount && !out) throw Error("sahara_gpu_pair_links: null output");
        std::copy_n(c->pairs.linkBuf.ptr, c->pairs.linkCount, out);
    });
}

uint32_t sahara_pair_mapq(const sahara_pair_summary* s, uint32_t n_best) {
    return s ? pairMapq(s->best, s->next, n_best) : 0u;
}

// (links and primaries are counted from the links, so an overflow re-run leaves the figures of the batches that count)
int sahara_gpu_pair_links_stats(void* ctx, sahara_pair_links_stats* stats) {
    return guarded([&] {
        if (!stats) throw Error("sahara_gpu_pair_links_stats: null output");
        const Ctx* c = ctxOf(ctx);
        sahara_pair_links_stats s{};
        if (c->pairs.linksOn) {
            s.links = c->pairs.linkCount;
            s.kernel_ms = c->stageStats.linkMs;
            for (uint64_t i = 0; i < c->pairs.linkCount; ++i) s.primaries += c->pairs.linkBuf.ptr[i].flags & kLinkPrimary;
        }
        *stats = s;
    });
}

int sahara_gpu_set_rescue(void* ctx, int on, uint32_t max_err, uint32_t max_anchors) {
    return guarded([&] {
        if (on && (max_err < 1 || max_err > SAHARA_ALIGN_MAX_ERR))
            throw Error("sahara_gpu_set_rescue: max_err must be in [1, " + std::to_string(SAHARA_ALIGN_MAX_ERR) + "]");
        Ctx* c = ctxOf(ctx);
        c->rescue.on = on != 0;
        c->rescue.maxErr = on ? max_err : 0u;
        c->rescue.maxAnchors = on ? max_anchors : 0u;
    });
}

int sahara_gpu_rescue_stats(void* ctx, sahara_rescue_stats* stats) {
    return guarded([&] {
        if (!stats) throw Error("sahara_gpu_rescue_stats: null output");
        *stats = ctxOf(ctx)->stageStats.rescue;
    });
}

int sahara_gpu_save(void* ctx, const char* path) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        const size_t np = c->more.size() + 1;
        std::vector<std::vector<uint8_t>> bf(np), br(np);
        std::vector<std::vector<uint64_t>> sb(np);
        std::vector<std::vector<uint32_t>> smp(np);
        std::vector<IdxParts> parts(np);
        for (uint32_t p = 0; p < np; ++p) {
            const DeviceIndex& D = partOf(c, p);
            const uint64_t n = D.n;
            bf[p].resize(n);
            br[p].resize(n);
            sb[p].resize(n / 64 + 1);
            smp[p].resize(D.nsamples);
            exportParts(D, bf[p].data(), br[p].data(), sb[p].data(), smp[p].data(), c->st);
            IdxParts& P = parts[p];
            P.sigma = D.sigma;
            P.n = n;
            P.rate = D.rate;
            std::copy(D.C, D.C + 8, P.C);
            P.recLens = D.recLens;
            P.bwtF = bf[p].data();
            P.bwtR = br[p].data();
            P.sampled = sb[p].data();
            P.samples = smp[p].data();
            P.nsamples = smp[p].size();
        }
        writeIdxAll(path, parts);
    });
}

int sahara_gpu_placement(void* ctx, int* device, int* numa_node, int* n_cpus) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (device) *device = c->device;
        if (numa_node) *numa_node = c->place.node;
        if (n_cpus) *n_cpus = c->place.ncpus;
    });
}

void sahara_gpu_close(void* ctx) {
    if (!ctx) return;
    Ctx* c = static_cast<Ctx*>(ctx);
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"
