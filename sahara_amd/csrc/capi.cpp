// capi.cpp — the search calls of libsahara_hip.so's C ABI (include/sahara_hip.h)
// and the host buffers their hits leave in. The context and index calls are
// in capi_ctx.cpp, alignment in capi_align.cpp, the synthetic-data and
// host-only helpers in capi_synth.cpp.
//
// The drop-in boundary for sahara's hot path: index residency
// (search.cpp:162-169), GPU index construction (index.cpp:87-100), and
// search + locate (search.cpp:218-250). No C++ types or exceptions cross it.

#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "ctx.h"

using namespace sahara;

namespace sahara {

bool hitLess(const sahara_hit& a, const sahara_hit& b) {
    if (a.qid != b.qid) return a.qid < b.qid;
    if (a.seq_id != b.seq_id) return a.seq_id < b.seq_id;
    if (a.pos != b.pos) return a.pos < b.pos;
    return a.err < b.err;
}

// --max_hits n (search_n / search_best_n, search.cpp:228,231,240). Upstream's
// counting rule is unverifiable offline; policy here: per query,
// the n distinct text positions (seq_id, pos) with the fewest errors, ties by
// (seq_id, pos), each reported once with its minimum error count. Input and
// output are in canonical (qid, seq_id, pos, err) order.
void limitHits(std::vector<sahara_hit>& v, uint32_t n) {
    size_t w = 0;
    std::vector<sahara_hit> q;
    for (size_t i = 0; i < v.size();) {
        size_t j = i;
        q.clear();
        for (; j < v.size() && v[j].qid == v[i].qid; ++j)
            if (q.empty() || q.back().seq_id != v[j].seq_id || q.back().pos != v[j].pos) q.push_back(v[j]);
        if (q.size() > n) {
            std::stable_sort(q.begin(), q.end(), [](const sahara_hit& a, const sahara_hit& b) { return a.err < b.err; });
            q.resize(n);
            std::sort(q.begin(), q.end(), hitLess);
        }
        for (auto& h : q) v[w++] = h;
        i = j;
    }
    v.resize(w);
}

void handOver(const std::vector<sahara_hit>& v, sahara_hit** hits, uint64_t* n_hits) {
    auto* buf = static_cast<sahara_hit*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(sahara_hit)));
    if (!buf) throw Error("out of host memory for hits");
    if (!v.empty()) std::memcpy(buf, v.data(), v.size() * sizeof(sahara_hit));
    *hits = buf;
    *n_hits = v.size();
}

// SAHARA_TIMING=2: a call's host-side marks (Ctx::mark), from t0 on, printed (stderr) at its end
static void traceBegin(Ctx* c, std::chrono::steady_clock::time_point t0) {
    const char* te = std::getenv("SAHARA_TIMING");
    c->traceOn = te && std::atoi(te) >= 2;
    c->traceT0 = t0;
    c->trace.clear();
}

// Hit buffers handed to the caller. Buffers of >= 64 MB are page-locked
// (hipHostMalloc), so the device-to-host copy runs at the link's rate straight
// into them, and sahara_gpu_free hands them back to a small pool instead of
// unpinning them: pinning (and first-touching) 0.6 GB costs more than copying
// into it, and a fresh box without transparent huge pages paid 28.6 ms for
// the page faults of a pageable buffer against 13 ms for the copy.
struct HitPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> live;       // pinned buffers the callers hold
    std::vector<std::pair<void*, size_t>> idle;   // pinned buffers ready for reuse
    static constexpr size_t kKeep = 2;
    // the size of an idle buffer that holds `bytes` (the last such), 0: none does
    size_t idleHolding(size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        size_t found = 0;
        for (auto& e : idle)
            if (e.second >= bytes) found = e.second;
        return found;
    }
};
static HitPool& hitPool() {
    static HitPool* p = new HitPool;  // never destroyed: callers may free after static destructors ran
    return *p;
}

// allocPinned (ctx.h): host buffer of `bytes` (released with sahara_gpu_free);
// *pinned tells whether the device can copy (or write) into it directly;
// *capBytes its size.

// Host buffer for n hits (released with sahara_gpu_free).
static void* allocHits(uint64_t n, bool* pinned, uint64_t* capHits = nullptr, bool mayPin = true) {
    size_t cap = 0;
    void* p = allocPinned(std::max<uint64_t>(n, 1) * sizeof(sahara_hit), pinned, &cap, mayPin);
    if (capHits) *capHits = cap / sizeof(sahara_hit);
    return p;
}

// always: pinned whatever the size (a sink the device writes into)
void* allocPinned(size_t bytes, bool* pinned, size_t* capBytes, bool mayPin, bool always) {
    bytes = std::max<size_t>(bytes, 1);
    *pinned = false;
    *capBytes = bytes;
    size_t pinMin = 64u << 20;  // SAHARA_PIN_MIN: smallest pinned buffer in bytes (tests pin every size)
    if (const char* e = std::getenv("SAHARA_PIN_MIN")) pinMin = (size_t)std::atoll(e);
    if (bytes < pinMin && !always) return std::malloc(bytes);
    HitPool& P = hitPool();
    std::vector<void*> unpin;
    void* p = nullptr;
    {
        std::lock_guard<std::mutex> g(P.mu);
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < P.idle.size(); ++i)
            if (P.idle[i].second >= bytes && (best == SIZE_MAX || P.idle[i].second < P.idle[best].second)) best = i;
        if (best != SIZE_MAX) {
            p = P.idle[best].first;
            P.live[p] = P.idle[best].second;
            *capBytes = P.idle[best].second;
            P.idle.erase(P.idle.begin() + (long)best);
        } else {  // none fits: the smaller idle ones will not fit later calls of this size either
            for (auto& e : P.idle) unpin.push_back(e.first);
            P.idle.clear();
        }
    }
    for (void* q : unpin) (void)hipHostFree(q);
    if (p) {
        *pinned = true;
        return p;
    }
    if (!mayPin) return std::malloc(bytes);  // a one-off caller: pinning would cost more than it saves
    const size_t huge = 2u << 20, cap = (bytes + bytes / 8 + huge - 1) / huge * huge;  // room for a run with more hits
    if (hipHostMalloc(&p, cap, hipHostMallocPortable) == hipSuccess && p) {
        std::lock_guard<std::mutex> g(P.mu);
        P.live[p] = cap;
        *pinned = true;
        *capBytes = cap;
        return p;
    }
    (void)hipGetLastError();
    p = std::aligned_alloc(huge, (bytes + huge - 1) / huge * huge);  // pageable fallback
    if (p) (void)madvise(p, (bytes + huge - 1) / huge * huge, MADV_HUGEPAGE);
    return p;
}

void freeHits(void* p) {
    if (!p) return;
    HitPool& P = hitPool();
    void* drop = nullptr;
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.live.find(p);
        if (it == P.live.end()) {
            std::free(p);
            return;
        }
        P.idle.emplace_back(p, it->second);
        P.live.erase(it);
        if (P.idle.size() > HitPool::kKeep) {
            drop = P.idle.front().first;
            P.idle.erase(P.idle.begin());
        }
    }
    if (drop) (void)hipHostFree(drop);
}

// memcpy from several threads (host copies out of the pinned staging chunks)
static void parallelCopy(void* dst, const void* src, size_t bytes) {
    const unsigned nt = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    if (bytes < (4u << 20) || nt == 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> ts;
    const size_t per = (bytes / nt + 4095) & ~size_t(4095);
    for (unsigned i = 0; i < nt; ++i) {
        const size_t b = i * per, e = std::min(bytes, b + per);
        if (b >= e) break;
        ts.emplace_back([=] { std::memcpy(static_cast<char*>(dst) + b, static_cast<const char*>(src) + b, e - b); });
    }
    for (auto& t : ts) t.join();
}

// Device hits -> pageable host memory through two pinned chunks: chunk k's
// DMA runs while the host copies chunk k-1 out (a direct copy to pageable
// memory runs at ~10 GB/s).
void copyOut(Ctx* c, void* dst, const void* src, size_t bytes) {
    if (bytes < (8u << 20)) {
        SH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return;
    }
    const size_t n = (bytes + Ctx::kOutChunk - 1) / Ctx::kOutChunk;
    auto len = [&](size_t k) { return std::min(Ctx::kOutChunk, bytes - k * Ctx::kOutChunk); };
    for (size_t k = 0; k <= n; ++k) {
        if (k < n) {
            SH_HIP(hipMemcpyAsync(c->outStage[k & 1].ptr, static_cast<const char*>(src) + k * Ctx::kOutChunk, len(k),
                                  hipMemcpyDeviceToHost, c->st));
            SH_HIP(hipEventRecord(c->outCopied[k & 1], c->st));
        }
        if (k > 0) {
            SH_HIP(hipEventSynchronize(c->outCopied[(k - 1) & 1]));
            parallelCopy(static_cast<char*>(dst) + (k - 1) * Ctx::kOutChunk, c->outStage[(k - 1) & 1].ptr, len(k - 1));
        }
    }
}

// Waits for every stream of the context (after a failed streamed search: the
// issued batches may still run and copy into the sink).
static void drainAll(Ctx* c) {
    drainPacking(c);  // chunks packed ahead: nothing reads the caller's buffer after the call
    for (const Stream* s : {&c->st, &c->stB, &c->stC, &c->stD, &c->stE, &c->stF})
        if (s->s) (void)hipStreamSynchronize(*s);
}

// SAHARA_TIMING=2: each chunk DMA's duration and rate from its events
static void printDmaTimes(Ctx* c) {
    for (size_t i = 0; i < c->dmaUsed; ++i) {
        float ms = 0;
        auto& d = c->dmaEv[i];
        if (hipEventElapsedTime(&ms, d.second.first, d.second.second) == hipSuccess)
            std::fprintf(stderr, "[sahara]   dma %zu: %.1f MB in %.3f ms, %.1f GB/s\n", i, d.first / 1e6, ms,
                         ms > 0 ? d.first / (ms * 1e6) : 0.0);
    }
    c->dmaUsed = 0;
}

// ... of a streamed call, with its DMA times
static void traceEnd(Ctx* c) {
    std::sort(c->trace.begin(), c->trace.end());
    for (auto& m : c->trace) std::fprintf(stderr, "[sahara]   %8.2f %s\n", m.first, m.second.c_str());
    printDmaTimes(c);
    c->traceOn = false;
}

ReadRows readRows(int reverse, uint64_t n_reads, uint64_t limit) {
    uint64_t npat = reverse ? 2 * n_reads : n_reads;
    if (limit && limit < npat) npat = limit;
    if (npat == 0) throw Error("no patterns");
    return {npat, reverse ? (npat + 1) / 2 : npat};
}

// The pair stage's refusals of a reads or packed call, before anything is staged (docs/semantics.md
// "Pairs"): the mates' reverse complements are what pairs with them, and the list holds whole pairs.
static void checkPairsReads(const Ctx* c, int reverse, const ReadRows& R, uint32_t len) {
    if (!c->pairs.on) return checkPairsCall(c, R.npat, len);  // (what needs pairs on is refused there)
    if (!reverse) throw Error("pairs: a reads call needs reverse != 0 (a mate pairs with its partner's reverse complement)");
    checkPairsCall(c, R.npat, len);
}

// Hits (or records) a call's sink is sized for: what the last call found and
// an eighth more (the bench's steady state), else 2 per pattern
static uint64_t sinkEstimate(const Ctx* c, uint64_t npat) {
    return c && c->lastHits ? c->lastHits + c->lastHits / 8 + 1024 : 2 * npat + 1024;
}

// A streamed call fails after staging (the guard of streamedCall): when this
// returns nothing of the call runs, reads the caller's queries or writes into
// its sink, which the caller's owner frees next (it is declared before the
// guard), and nothing stays staged.
// packingOnly: no pass was started, only chunks may be packing ahead.
static void abandonCall(Ctx* c, bool packingOnly) {
    if (packingOnly) drainPacking(c);
    else drainAll(c);
    if (c->sk.route == HitRoute::Expander) {
        try {
            c->expander->drain();
        } catch (...) {
        }
    }
    c->sk = {};
}

// The scheme(s) of a call: one, or the exact-j schemes of a besthits call back
// to back, which the pass runs as rounds within each batch (pass.cpp).
struct Schemes {
    const uint32_t *pi, *l, *u;
    const uint32_t* ns;  // rows of each
    uint32_t n;
    int edit;
    uint64_t rows() const {
        uint64_t t = 0;
        for (uint32_t j = 0; j < n; ++j) t += ns[j];
        return t;
    }
};

// The queries of a streamed call: `rows` source rows of `len` symbols (ranks,
// or 2-bit codes with `packed`), which make npat patterns (rc: each row and
// its reverse complement).
struct Queries {
    const uint8_t* src;
    uint64_t rows;
    bool rc;
    uint64_t npat;
    uint32_t len;
    const PackedReads* packed;
};

using clk = std::chrono::steady_clock;
static double msBetween(clk::time_point a, clk::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}
struct CallTimes {
    clk::time_point start, staged, sinkOpen, passDone;
};

// The two shapes in which a streamed call's hits leave (streamedCall below).
// Each opens its sink before the pass: the host buffer, c->sk.host / cap and
// the route; and collects after it: whatever the sink did not take during
// the pass, then the hand-over to the caller. The buffer belongs to the shape,
// which the caller declares before the driver's guard: it is freed after
// everything that could write into it has stopped.

// Whole hits, returned as sahara_hit** (sahara_gpu_search and its kin): each
// batch's hits into a pooled host buffer during the pass (hit_route.h
// callRoute), the rest after it.
struct WholeHits {
    uint32_t maxHits;
    sahara_hit** hits;
    uint64_t* nHits;
    HostBuf sink{nullptr, freeHits};
    bool pinned = false;     // the device copies into `sink` directly
    bool hostLimit = false;  // --max_hits on the merged hits of a multi-part index (limitHits)

    void openSink(Ctx* c, uint64_t npat) {
        // --max_hits: per batch on the device (limitBatch), so the limited hits
        // stream to the host like any others; a multi-part index limits after
        // its parts merge, on the host (limitHits)
        hostLimit = maxHits && !c->more.empty();
        c->sk.limitN = hostLimit ? 0u : maxHits;
        if (hostLimit) return;
        // a first call takes a pooled buffer if there is one, but pins none:
        // pinning ~1 GB costs ~200 ms, ten times the pageable copy-out
        uint64_t cap = 0;
        HostBuf p(allocHits(sinkEstimate(c, npat), &pinned, &cap, c->lastHits != 0), freeHits);
        const bool compactOk = c->downRing.ptr && c->maxErr < 16 && c->I.n < (1ull << 32);
        const char* fe = std::getenv("SAHARA_FULL_DOWNLOAD");
        const char* ce = std::getenv("SAHARA_COMPACT_DOWNLOAD");
        const CallRoute r = callRoute(pinned, compactOk, fe && std::atoi(fe), ce && std::atoi(ce));
        if (!p || r.route == HitRoute::Device) return;  // no sink: every hit goes after the pass
        if (r.route == HitRoute::Expander) {
            if (!c->expander)
                c->expander = std::make_unique<Expander>(c->device, hostThreads(c, 8) - 1, &c->place);
            c->expander->setStarts(&c->I.recStarts);
            c->expander->mark = [c](const char* w, uint64_t i) { c->mark(w, i); };
            c->expander->reset();
        }
        sink = std::move(p);
        c->sk.host = sink.get();
        c->sk.cap = cap;
        c->sk.route = r.route;
        c->sk.wholeFallback = r.wholeFallback;
    }

    void collect(Ctx* c) {
        if (hostLimit) {
            std::vector<sahara_hit> v(c->nout);
            if (c->nout) SH_HIP(hipMemcpy(v.data(), c->wholeHits(), c->nout * sizeof(sahara_hit), hipMemcpyDeviceToHost));
            limitHits(v, maxHits);
            return handOver(v, hits, nHits);
        }
        if (sink && c->nout > c->sk.cap) sink.reset();  // more hits than the sink holds: a bigger buffer, copied whole
        if (!sink) {
            c->sk.done = 0;
            sink.reset(allocHits(c->nout, &pinned, nullptr, c->lastHits != 0));
            if (!sink) throw Error("out of host memory for hits");
        }
        sahara_hit* buf = static_cast<sahara_hit*>(sink.get());
        if (c->nout > c->sk.done) {  // the rest (or all) of the hits
            const size_t bytes = (c->nout - c->sk.done) * sizeof(sahara_hit);
            const sahara_hit* src = c->wholeHits() + c->sk.done;
            if (pinned) {
                SH_HIP(hipMemcpyAsync(buf + c->sk.done, src, bytes, hipMemcpyDeviceToHost, c->st));
                SH_HIP(hipStreamSynchronize(c->st));
            } else {
                copyOut(c, buf + c->sk.done, src, bytes);
            }
        }
        *hits = static_cast<sahara_hit*>(sink.release());
        *nHits = c->nout;
    }

    void timing(const Ctx* c, const CallTimes& t) const {  // where a call's wall time goes
        std::fprintf(stderr, "[sahara] stage %.1f ms, sink %.1f ms, pass %.1f ms (host packing %.1f ms), output %.1f ms\n",
                     msBetween(t.start, t.staged), msBetween(t.staged, t.sinkOpen), msBetween(t.sinkOpen, t.passDone),
                     c->up.hostMs, c->stats.output_ms);
    }
};

// Records in blocks, returned as sahara_hit_blocks (the compact calls): every
// batch's hits as 8-B records, copied by the device into a pinned host buffer
// (pass.cpp sinkBatch), handed over as blocks (one per batch).
struct BlockRecs {
    sahara_hit_blocks* out;
    HostBuf recs{nullptr, freeHits};
    uint64_t recCap = 0;

    // the sink, sized from the last call (else 2 hits per pattern), always
    // page-locked: the device writes into it
    void openSink(Ctx* c, uint64_t npat) {
        bool pinned = false;
        size_t capBytes = 0;
        recs.reset(allocPinned(sinkEstimate(c, npat) * 8, &pinned, &capBytes, true, true));
        if (!recs) throw Error("out of host memory for hits");
        c->sk.route = HitRoute::Records;
        c->sk.host = pinned ? recs.get() : nullptr;
        c->sk.cap = pinned ? capBytes / 8 : 0;
        // SAHARA_SINK_RECORDS: the sink takes no more records than this during the pass (a test hook: pinned
        // buffers come in 2 MB steps, so a small call's sink is never too small, and collect's refill never runs)
        if (const char* e = std::getenv("SAHARA_SINK_RECORDS")) c->sk.cap = std::min<uint64_t>(c->sk.cap, std::strtoull(e, nullptr, 10));
        if (c->sk.cap) c->reserveRecs(c->sk.cap);
        recCap = capBytes / 8;
    }

    void collect(Ctx* c) {
        if (!c->sk.host || c->sk.done < c->nout) {
            // the sink held too few (or is not pinned): the records of every
            // batch again, from the device-resident records (c->outRecs holds the
            // whole call's: pass.cpp finish), into one that fits
            if (c->nout > recCap) {
                bool pinned = false;
                size_t capBytes = 0;
                recs.reset();
                recs.reset(allocPinned(c->nout * 8, &pinned, &capBytes, true, true));
                if (!recs) throw Error("out of host memory for hits");
            }
            uint64_t b0 = 0;
            for (size_t b = 0; b < c->batchQ0.size(); b0 = c->batchEnd[b], ++b)
                if (!c->batchDirect[b])  // (a batch of 2^28 queries or more: whole hits in c->out)
                    launchCompactHits(c->out.ptr + b0, c->batchEnd[b] - b0, c->batchQ0[b], c->I.dRecStarts.ptr,
                                      c->outRecs.ptr + b0, c->st);
            if (c->nout) SH_HIP(hipMemcpyAsync(recs.get(), c->outRecs.ptr, c->nout * 8, hipMemcpyDeviceToHost, c->st));
            SH_HIP(hipStreamSynchronize(c->st));
        }
        const size_t nb = c->batchQ0.size();
        HostBuf q0(std::malloc(std::max<size_t>(nb, 1) * 8), std::free);
        HostBuf end(std::malloc(std::max<size_t>(nb, 1) * 8), std::free);
        if (!q0 || !end) throw Error("out of host memory for hit blocks");
        if (nb) std::memcpy(q0.get(), c->batchQ0.data(), nb * 8);
        if (nb) std::memcpy(end.get(), c->batchEnd.data(), nb * 8);
        if (c->recStartsEnd.size() != c->I.recStarts.size() + 1) {
            c->recStartsEnd = c->I.recStarts;
            c->recStartsEnd.push_back(c->I.n);
        }
        out->recs = static_cast<uint64_t*>(recs.release());
        out->n_hits = c->nout;
        out->block_qid0 = static_cast<uint64_t*>(q0.release());
        out->block_end = static_cast<uint64_t*>(end.release());
        out->n_blocks = nb;
        out->rec_starts = c->recStartsEnd.data();
        out->n_records = c->I.recStarts.size();
    }

    void timing(const Ctx* c, const CallTimes& t) const {
        std::fprintf(stderr, "[sahara] compact call %.1f ms (host packing %.1f ms), output %.1f ms\n",
                     msBetween(t.start, clk::now()), c->up.hostMs, c->stats.output_ms);
    }
};

// Every streamed search call (search.cpp:218-250 from host queries to host
// hits): the streamed upload, the pipelined pass with each batch's hits on
// their way to the host while later batches search, then what is left of
// them, in the shape `out` (declared by the caller, so that its buffer
// outlives the guard here).
template <typename Out>
static void streamedCall(Ctx* c, const Queries& q, const Schemes& sc, Out& out) {
    CallTimes t{};
    t.start = clk::now();
    traceBegin(c, t.start);
    stageStreamed(c, q.src, q.rows, q.rc, q.npat, q.len, sc.pi, sc.l, sc.u, sc.ns, sc.n, sc.edit, q.packed);
    // (until the pass starts only the packing can be reading the caller's queries)
    bool passStarted = false;
    ScopeExit failed([&] { abandonCall(c, !passStarted); });
    t.staged = clk::now();
    out.openSink(c, q.npat);
    t.sinkOpen = clk::now();
    passStarted = true;
    run(c, false);
    c->sk.limitN = 0;
    uint32_t bad = 0;
    SH_HIP(hipMemcpy(&bad, c->badFlag.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (bad) throw Error("pattern rank out of range for this index");
    if (c->sk.route == HitRoute::Expander) c->expander->drain();
    c->mark("run end", 0);
    t.passDone = clk::now();
    out.collect(c);
    c->stats.output_ms = msBetween(t.passDone, clk::now());
    failed.dismiss();
    c->sk.route = HitRoute::Device;  // the pass is over: the sink is the caller's
    c->sk.wholeFallback = false;
    c->sk.host = nullptr;
    c->sk.streaming = false;  // every chunk is up: sahara_gpu_run may re-run the staged patterns
    c->stats.stage_ms = c->up.hostMs;
    for (int b = 0; b < 3; ++b) c->stats.upload_chunks[b] = c->up.chunks[b];
    c->lastHits = c->nout;
    if (std::getenv("SAHARA_TIMING")) {
        out.timing(c, t);
        traceEnd(c);
    }
}

static void searchWhole(Ctx* c, const Queries& q, const Schemes& sc, uint32_t max_hits, sahara_hit** hits,
                        uint64_t* n_hits) {
    if (max_hits && c->pairs.links)  // (docs/semantics.md "Pair links", refused calls)
        throw Error("pair links: a call with max_hits is not supported (the cut would drop linked hits)");
    WholeHits out{max_hits, hits, n_hits};
    streamedCall(c, q, sc, out);
}

// The compact calls refuse before staging: a refused call stages nothing.
static void searchBlocks(Ctx* c, const uint8_t* reads, uint64_t n_reads, uint32_t len, int reverse, uint64_t limit,
                         const Schemes& sc, sahara_hit_blocks* blocks, const PackedReads* packed = nullptr) {
    if (c->I.sigma != 5 && c->I.sigma != 6) throw Error("reverse complements need a dna4 or dna5 index");
    if (!c->more.empty()) throw Error("compact hit records need a single-part index (text < 2^32 symbols)");
    const ReadRows R = readRows(reverse, n_reads, limit);
    checkPairsReads(c, reverse, R, len);
    for (uint64_t i = 0, n = sc.rows() * len; i < n; ++i)
        if (sc.u[i] > 15) throw Error("compact hit records hold at most 15 errors");
    BlockRecs out{blocks};
    streamedCall(c, Queries{reads, R.rows, reverse != 0, R.npat, len, packed}, sc, out);
}

// besthits on the host: a loop over the exact-j schemes, each a whole
// device-resident pass over the patterns still without a hit, the found
// patterns marked and the rest subset here (search_ng21::search_best,
// search.cpp:233-241). The path of a multi-part index, where "found" is
// decided across the parts, and of SAHARA_BEST_HOST=1 (A/B and parity hook);
// a single-part index runs the schemes as rounds inside each batch of one
// streamed pass (pass.cpp).
static void bestOnHost(Ctx* c, const uint8_t* ranks, uint64_t n_patterns, uint32_t len, const Schemes& sc,
                       uint32_t max_hits, sahara_hit** hits, uint64_t* n_hits) {
    if (c->pairs.links) throw Error("pair links: besthits on the host is not supported (its hits are merged on the host)");
    std::vector<uint64_t> todo(n_patterns);
    for (uint64_t i = 0; i < n_patterns; ++i) todo[i] = i;
    std::vector<uint8_t> sub;
    std::vector<sahara_hit> all;
    sahara_stats acc{};
    sahara_loci_stats lociAcc{};  // (each pass below is a run of its own: the call's figures are their sums)
    // Pairs: a stratum whose hits all lack a mate would leave its queries "not found" here and let them
    // fall through to the next scheme, where the rounds of a streamed pass fix the stratum first.
    if (c->pairs.on)
        throw Error("pairs: besthits as a host loop of one pass per scheme (a multi-part index, SAHARA_BEST_HOST=1) "
                    "is not supported with pairs on");
    uint64_t off = 0;
    for (uint32_t j = 0; j < sc.n && !todo.empty(); off += (uint64_t)sc.ns[j] * len, ++j) {
        const uint8_t* src = ranks;
        if (todo.size() != n_patterns) {
            sub.resize(todo.size() * len);
            for (size_t i = 0; i < todo.size(); ++i)
                std::memcpy(sub.data() + i * len, ranks + todo[i] * len, len);
            src = sub.data();
        }
        stage(c, src, todo.size(), len, sc.pi + off, sc.l + off, sc.u + off, &sc.ns[j], 1, 1);
        // --max_hits per batch on the device (single part; the host pass
        // below is then a no-op on what is left)
        c->sk.limitN = c->more.empty() ? max_hits : 0u;
        {
            const ScopeExit limitOff([c] { c->sk.limitN = 0; });
            run(c, false);
        }
        std::vector<sahara_hit> v(c->nout);
        if (c->nout) SH_HIP(hipMemcpy(v.data(), c->out.ptr, c->nout * sizeof(sahara_hit), hipMemcpyDeviceToHost));
        acc.search_ms += c->stats.search_ms;
        acc.locate_ms += c->stats.locate_ms;
        acc.sort_ms += c->stats.sort_ms;
        acc.total_ms += c->stats.total_ms;
        acc.hits += c->stats.hits;
        acc.patterns += c->stats.patterns;
        lociAcc.hits_in += c->stageStats.loci.hits_in;
        lociAcc.loci += c->stageStats.loci.loci;
        lociAcc.batches += c->stageStats.loci.batches;
        lociAcc.kernel_ms += c->stageStats.loci.kernel_ms;
        std::vector<char> found(todo.size(), 0);
        for (auto& h : v) {
            found[h.qid] = 1;
            h.qid = todo[h.qid];
        }
        all.insert(all.end(), v.begin(), v.end());
        size_t w = 0;
        for (size_t i = 0; i < todo.size(); ++i)
            if (!found[i]) todo[w++] = todo[i];
        todo.resize(w);
    }
    c->stats = acc;
    c->stageStats.loci = lociAcc;
    std::sort(all.begin(), all.end(), hitLess);
    if (max_hits) limitHits(all, max_hits);
    handOver(all, hits, n_hits);
}

static bool bestHostForced() {
    const char* e = std::getenv("SAHARA_BEST_HOST");
    return e && std::atoi(e) != 0;
}

// The query list of a reads call as ranks on the host (the host loop's
// input): the reads, given one rank per byte or (packed) two bits per symbol
// with the N positions listed, interleaved with their reverse complements
// (reverse) and cut to R.npat patterns.
static std::vector<uint8_t> queryRanks(const Ctx* c, const uint8_t* src, uint32_t len, bool reverse, const ReadRows& R,
                                       const PackedReads* packed) {
    const uint32_t sigma = c->I.sigma;
    if (sigma != 5 && sigma != 6) throw Error("reverse complements need a dna4 or dna5 index");
    std::vector<uint8_t> reads;
    if (packed) {
        const uint8_t rankOf[4] = {1, 2, 3, (uint8_t)(sigma == 6 ? 5 : 4)};
        reads.resize(R.rows * len);
        for (uint64_t i = 0; i < reads.size(); ++i) {
            const uint64_t s = packed->sym0 + i;
            reads[i] = rankOf[(src[s / 4] >> (2 * (s % 4))) & 3u];
        }
        const uint64_t lo = packed->sym0, hi = lo + reads.size();
        for (uint64_t i = 0; i < packed->nCount; ++i) {
            if (i && packed->nPos[i] <= packed->nPos[i - 1])
                throw Error("N positions of packed reads must be strictly ascending");
            if (packed->nPos[i] < lo || packed->nPos[i] >= hi) continue;
            if (sigma == 5) throw Error("pattern rank out of range for this index");  // N is no dna4 rank
            reads[packed->nPos[i] - lo] = 4;
        }
        src = reads.data();
    }
    if (!reverse) return packed ? std::move(reads) : std::vector<uint8_t>(src, src + R.npat * len);
    std::vector<uint8_t> both(2 * R.rows * len);
    if (sahara_interleave_rc(src, R.rows, len, sigma, both.data()) != 0) throw Error(g_err);
    both.resize(R.npat * len);
    return both;
}

// The besthits twins of the reads calls: whole hits ...
static void bestStreamed(Ctx* c, const uint8_t* src, uint64_t n_reads, uint32_t len, bool interleave, int reverse,
                         uint64_t limit, const Schemes& sc, uint32_t max_hits, sahara_hit** hits, uint64_t* n_hits,
                         const PackedReads* packed) {
    if (!sc.n) throw Error("besthits: no schemes");
    const ReadRows R = interleave ? readRows(reverse, n_reads, limit) : ReadRows{n_reads, n_reads};
    if (R.npat == 0) throw Error("no patterns");
    if (interleave) checkPairsReads(c, reverse, R, len);
    else checkPairsCall(c, R.npat, len);
    const bool rc = interleave && reverse != 0;
    if (c->more.empty() && !bestHostForced()) {
        if (interleave && !packed && c->I.sigma != 5 && c->I.sigma != 6)
            throw Error("reverse complements need a dna4 or dna5 index");
        return searchWhole(c, Queries{src, R.rows, rc, R.npat, len, packed}, sc, max_hits, hits, n_hits);
    }
    if (!interleave) return bestOnHost(c, src, R.npat, len, sc, max_hits, hits, n_hits);
    const std::vector<uint8_t> ranks = queryRanks(c, src, len, rc, R, packed);
    bestOnHost(c, ranks.data(), R.npat, len, sc, max_hits, hits, n_hits);
}

}  // namespace sahara

extern "C" {

int sahara_gpu_stage(void* ctx, const uint8_t* ranks, uint64_t n_patterns, uint32_t len, const uint32_t* pi,
                     const uint32_t* l, const uint32_t* u, uint32_t n_searches, int edit) {
    return guarded([&] {
        checkPairsCall(ctxOf(ctx), n_patterns, len);
        stage(ctxOf(ctx), ranks, n_patterns, len, pi, l, u, &n_searches, 1, edit);
    });
}

int sahara_gpu_run(void* ctx, int count, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        traceBegin(c, std::chrono::steady_clock::now());
        run(c, count != 0);
        if (n_hits) *n_hits = c->nout;
        if (c->traceOn) {
            c->mark("run returns", 0);
            std::sort(c->trace.begin(), c->trace.end());
            for (auto& m : c->trace) std::fprintf(stderr, "[sahara]   %8.3f %s\n", m.first, m.second.c_str());
            c->traceOn = false;
        }
    });
}

int sahara_gpu_fetch(void* ctx, sahara_hit* out, uint64_t capacity, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (n_hits) *n_hits = c->nout;
        if (capacity < c->nout) throw Error("sahara_gpu_fetch: capacity too small");
        if (c->nout) SH_HIP(hipMemcpy(out, c->wholeHits(), c->nout * sizeof(sahara_hit), hipMemcpyDeviceToHost));
    });
}

int sahara_gpu_copy_hits(void* ctx, void* dst_device, uint64_t capacity, uint64_t qid_offset, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (n_hits) *n_hits = c->nout;
        if (capacity < c->nout) throw Error("sahara_gpu_copy_hits: capacity too small");
        if (c->nout && !dst_device) throw Error("sahara_gpu_copy_hits: null destination");
        launchCopyHits(c->wholeHits(), c->nout, qid_offset, static_cast<sahara_hit*>(dst_device), c->st);
        SH_HIP(hipStreamSynchronize(c->st));
    });
}

int sahara_gpu_digest(void* ctx, uint64_t* digest) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        SH_HIP(hipMemsetAsync(c->counters.ptr + 4, 0, 8, c->st));
        launchDigest(c->wholeHits(), c->nout, c->counters.ptr + 4, c->st);
        unsigned long long d = 0;
        SH_HIP(hipMemcpyAsync(&d, c->counters.ptr + 4, 8, hipMemcpyDeviceToHost, c->st));
        SH_HIP(hipStreamSynchronize(c->st));
        *digest = d;
    });
}

int sahara_gpu_stats(void* ctx, sahara_stats* stats) {
    return guarded([&] { *stats = ctxOf(ctx)->stats; });
}

int sahara_gpu_search(void* ctx, const uint8_t* ranks, uint64_t n_patterns, uint32_t len, const uint32_t* pi,
                      const uint32_t* l, const uint32_t* u, uint32_t n_searches, int edit, uint32_t max_hits,
                      sahara_hit** hits, uint64_t* n_hits) {
    return guarded([&] {
        checkPairsCall(ctxOf(ctx), n_patterns, len);
        searchWhole(ctxOf(ctx), Queries{ranks, n_patterns, false, n_patterns, len, nullptr},
                    Schemes{pi, l, u, &n_searches, 1, edit}, max_hits, hits, n_hits);
    });
}

int sahara_gpu_search_reads(void* ctx, const uint8_t* reads, uint64_t n_reads, uint32_t len, int reverse,
                            uint64_t limit, const uint32_t* pi, const uint32_t* l, const uint32_t* u,
                            uint32_t n_searches, int edit, uint32_t max_hits, sahara_hit** hits, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (c->I.sigma != 5 && c->I.sigma != 6) throw Error("reverse complements need a dna4 or dna5 index");
        const ReadRows R = readRows(reverse, n_reads, limit);
        checkPairsReads(c, reverse, R, len);
        searchWhole(c, Queries{reads, R.rows, reverse != 0, R.npat, len, nullptr}, Schemes{pi, l, u, &n_searches, 1, edit},
                    max_hits, hits, n_hits);
    });
}

int sahara_gpu_search_reads_compact(void* ctx, const uint8_t* reads, uint64_t n_reads, uint32_t len, int reverse,
                                    uint64_t limit, const uint32_t* pi, const uint32_t* l, const uint32_t* u,
                                    uint32_t n_searches, int edit, sahara_hit_blocks* out) {
    return guarded([&] {
        if (!out) throw Error("sahara_gpu_search_reads_compact: null output");
        *out = sahara_hit_blocks{};
        searchBlocks(ctxOf(ctx), reads, n_reads, len, reverse, limit, Schemes{pi, l, u, &n_searches, 1, edit}, out);
    });
}

int sahara_gpu_search_packed(void* ctx, const uint8_t* codes, uint64_t sym0, const uint64_t* n_pos, uint64_t n_count,
                             uint64_t n_reads, uint32_t len, int reverse, uint64_t limit, const uint32_t* pi,
                             const uint32_t* l, const uint32_t* u, uint32_t n_searches, int edit, uint32_t max_hits,
                             sahara_hit** hits, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!codes || (n_count && !n_pos)) throw Error("sahara_gpu_search_packed: null input");
        const ReadRows R = readRows(reverse, n_reads, limit);
        checkPairsReads(c, reverse, R, len);
        const PackedReads pk{sym0, n_pos, n_count};
        searchWhole(c, Queries{codes, R.rows, reverse != 0, R.npat, len, &pk}, Schemes{pi, l, u, &n_searches, 1, edit},
                    max_hits, hits, n_hits);
    });
}

int sahara_gpu_search_packed_compact(void* ctx, const uint8_t* codes, uint64_t sym0, const uint64_t* n_pos,
                                     uint64_t n_count, uint64_t n_reads, uint32_t len, int reverse, uint64_t limit,
                                     const uint32_t* pi, const uint32_t* l, const uint32_t* u, uint32_t n_searches,
                                     int edit, sahara_hit_blocks* out) {
    return guarded([&] {
        if (!out) throw Error("sahara_gpu_search_packed_compact: null output");
        *out = sahara_hit_blocks{};
        if (!codes || (n_count && !n_pos)) throw Error("sahara_gpu_search_packed_compact: null input");
        const PackedReads pk{sym0, n_pos, n_count};
        searchBlocks(ctxOf(ctx), codes, n_reads, len, reverse, limit, Schemes{pi, l, u, &n_searches, 1, edit}, out, &pk);
    });
}

int sahara_gpu_prepare(void* ctx, uint64_t n_patterns, uint32_t len) {
    return guarded([&] {
        if (n_patterns == 0) return;
        Ctx* c = ctx ? ctxOf(ctx) : nullptr;
        if (c) SH_HIP(hipSetDevice(c->device));
        // the sink the first compact call asks the pool for (BlockRecs::openSink),
        // pinned now and handed back to the pool, where the call finds it
        const uint64_t est = sinkEstimate(c, n_patterns);
        size_t capBytes = hitPool().idleHolding(est * 8);  // pinned already (a NULL-context call before)
        bool pinned = capBytes != 0;
        if (!pinned) {
            void* p = allocPinned(est * 8, &pinned, &capBytes, true, true);
            if (!p) throw Error("out of host memory for hits");
            freeHits(p);
        }
        if (!c) return;  // (NULL context: the host part only, e.g. beside the index load)
        if (pinned) c->reserveRecs(capBytes / 8);
        c->out.reserve(est);
        // the slots and the locate chain's buffers of a streamed pass, from
        // the pass's own sizing (pass.cpp; the keys sized for a batch's rows
        // at four per pattern, grown by the pass if short)
        const PassKnobs k = readPassKnobs(c->verify);
        const uint64_t maxBatch = maxBatchOf(std::nullopt, true, 1, false);
        initWorkCaps(c, maxBatch, k);
        const uint64_t nb = std::min<uint64_t>((n_patterns + maxBatch - 1) / maxBatch, Ctx::kSlots);
        reserveLocate(c, maxBatch, nb);
        c->partial.reserve(scanTiles((uint32_t)maxBatch));
        c->k0.reserve(std::min<uint64_t>(n_patterns, maxBatch) * 4);
        for (uint64_t i = 0; i < nb; ++i) reserveSlot(c, c->slot[i]);
        if (len) {
            const uint64_t patWords = (len + 7) / 8, patBlocks = (len + 31) / 32;
            c->rawPats.reserve(n_patterns * len);
            c->pats.reserve(n_patterns * patWords + 4);
            c->pats3.reserve(n_patterns * patBlocks);
            c->readRaw.reserve((n_patterns + 1) / 2 * len);
            c->nibPats.reserve((n_patterns * len + 1) / 2 + 16);  // the streamed upload's staging (staging.cpp)
        }
    });
}

void sahara_gpu_free_blocks(sahara_hit_blocks* b) {
    if (!b) return;
    freeHits(b->recs);
    std::free(b->block_qid0);
    std::free(b->block_end);
    *b = sahara_hit_blocks{};
}

int sahara_gpu_search_best(void* ctx, const uint8_t* ranks, uint64_t n_patterns, uint32_t len, const uint32_t* pi,
                           const uint32_t* l, const uint32_t* u, const uint32_t* n_searches, uint32_t n_schemes,
                           uint32_t max_hits, sahara_hit** hits, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!n_schemes) throw Error("sahara_gpu_search_best: no schemes");
        bestStreamed(c, ranks, n_patterns, len, false, 0, 0, Schemes{pi, l, u, n_searches, n_schemes, 1}, max_hits, hits,
                     n_hits, nullptr);
    });
}

int sahara_gpu_search_best_reads(void* ctx, const uint8_t* reads, uint64_t n_reads, uint32_t len, int reverse,
                                 uint64_t limit, const uint32_t* pi, const uint32_t* l, const uint32_t* u,
                                 const uint32_t* n_searches, uint32_t n_schemes, uint32_t max_hits, sahara_hit** hits,
                                 uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!reads) throw Error("sahara_gpu_search_best_reads: null input");
        bestStreamed(c, reads, n_reads, len, true, reverse, limit, Schemes{pi, l, u, n_searches, n_schemes, 1}, max_hits,
                     hits, n_hits, nullptr);
    });
}

int sahara_gpu_search_best_packed(void* ctx, const uint8_t* codes, uint64_t sym0, const uint64_t* n_pos,
                                  uint64_t n_count, uint64_t n_reads, uint32_t len, int reverse, uint64_t limit,
                                  const uint32_t* pi, const uint32_t* l, const uint32_t* u, const uint32_t* n_searches,
                                  uint32_t n_schemes, uint32_t max_hits, sahara_hit** hits, uint64_t* n_hits) {
    return guarded([&] {
        Ctx* c = ctxOf(ctx);
        if (!codes || (n_count && !n_pos)) throw Error("sahara_gpu_search_best_packed: null input");
        const PackedReads pk{sym0, n_pos, n_count};
        bestStreamed(c, codes, n_reads, len, true, reverse, limit, Schemes{pi, l, u, n_searches, n_schemes, 1}, max_hits,
                     hits, n_hits, &pk);
    });
}

// ... and compact records (single-part index: the rounds, always)
int sahara_gpu_search_best_packed_compact(void* ctx, const uint8_t* codes, uint64_t sym0, const uint64_t* n_pos,
                                          uint64_t n_count, uint64_t n_reads, uint32_t len, int reverse,
                                          uint64_t limit, const uint32_t* pi, const uint32_t* l, const uint32_t* u,
                                          const uint32_t* n_searches, uint32_t n_schemes, sahara_hit_blocks* out) {
    return guarded([&] {
        if (!out) throw Error("sahara_gpu_search_best_packed_compact: null output");
        *out = sahara_hit_blocks{};
        Ctx* c = ctxOf(ctx);
        if (!codes || (n_count && !n_pos)) throw Error("sahara_gpu_search_best_packed_compact: null input");
        if (!n_schemes) throw Error("besthits: no schemes");
        const PackedReads pk{sym0, n_pos, n_count};
        searchBlocks(c, codes, n_reads, len, reverse, limit, Schemes{pi, l, u, n_searches, n_schemes, 1}, out, &pk);
    });
}

void sahara_gpu_free(void* p) { freeHits(p); }

void* sahara_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        g_err = "could not allocate " + std::to_string(bytes) + " bytes of page-locked host memory";
        return nullptr;
    }
    return p;
}

void sahara_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

}  // extern "C"
