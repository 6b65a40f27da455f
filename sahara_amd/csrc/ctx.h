// ctx.h — the per-device context of libsahara_hip.so and what the C ABI
// (capi*.cpp), the query staging (staging.cpp) and the batch pipeline
// (pass.cpp) share.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sahara_hip.h"
#include "compact_hit.h"
#include "device_index.h"
#include "hit_route.h"
#include "host_pool.h"
#include "pass_plan.h"
#include "search.h"

namespace sahara {

extern thread_local std::string g_err;  // sahara_gpu_last_error

// Host side of sahara_gpu_search's compact hit download: batch by batch, the
// 8-B records (hits.hip kCompactHits) land in pinned staging memory on
// stream stF, and this thread expands them into the caller's sahara_hit
// buffer (record id by binary search over the record starts) on a few worker
// threads while later batches still search. Cuts the PCIe download to a third
// (8 of 24 B per hit).
class Expander {
public:
    struct Job {
        hipEvent_t ev;           // the batch's download is done
        const uint64_t* src;     // compact records (pinned staging)
        sahara_hit* dst;
        uint64_t n, q0;          // records; the batch's first qid
    };
    Expander(int device, unsigned workers, const Placement* pl) : device_(device), pool_(workers, pl) {
        th_ = std::thread([this, pl] {
            if (pl) pl->bind();
            loop();
        });
    }
    ~Expander() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void setStarts(const std::vector<uint64_t>* starts) { starts_ = starts; }
    std::function<void(const char*, uint64_t)> mark;  // SAHARA_TIMING=2 trace
    void submit(const Job& j) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(j);
            ++submitted_;
        }
        cv_.notify_all();
    }
    // waits until the first n jobs submitted since reset() are expanded
    void waitFor(uint64_t n) {
        std::unique_lock<std::mutex> lk(mu_);
        idle_.wait(lk, [&] { return done_ >= n || err_; });
    }
    void reset() {
        drain();
        std::lock_guard<std::mutex> g(mu_);
        submitted_ = done_ = 0;
    }
    // waits until every submitted batch is expanded; rethrows the first failure
    void drain() {
        std::unique_lock<std::mutex> lk(mu_);
        idle_.wait(lk, [&] { return q_.empty() && !busy_; });
        if (err_) {
            std::exception_ptr e = err_;
            err_ = nullptr;
            std::rethrow_exception(e);
        }
    }

private:
    void loop() {
        (void)hipSetDevice(device_);
        for (;;) {
            Job j{};
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                j = q_.front();
                q_.erase(q_.begin());
                busy_ = true;
            }
            try {
                SH_HIP(hipEventSynchronize(j.ev));
                if (mark) mark("expand", done_);
                expand(j);
                if (mark) mark("expanded", done_);
            } catch (...) {
                std::lock_guard<std::mutex> g(mu_);
                if (!err_) err_ = std::current_exception();
            }
            std::lock_guard<std::mutex> g(mu_);
            busy_ = false;
            ++done_;
            idle_.notify_all();
        }
    }
    void expand(const Job& j) {
        const std::vector<uint64_t>& S = *starts_;
        const unsigned nt = pool_.size();
        const uint64_t per = (j.n + nt - 1) / nt;
        pool_.run([&](unsigned t) {
            const uint64_t b = std::min(j.n, (uint64_t)t * per), e = std::min(j.n, b + per);
            sahara_compact::RecordCursor rec(S.data(), S.size());
            for (uint64_t i = b; i < e; ++i) {
                const uint64_t v = j.src[i];
                sahara_hit& h = j.dst[i];
                h.pos = rec.seek(sahara_compact::textOf(v));
                h.qid = j.q0 + sahara_compact::qidOf(v);
                h.seq_id = (uint32_t)rec.seq;
                h.err = sahara_compact::errOf(v);
            }
        });
    }
    int device_;
    HostPool pool_;
    const std::vector<uint64_t>* starts_ = nullptr;
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    std::vector<Job> q_;
    bool stop_ = false, busy_ = false;
    uint64_t submitted_ = 0, done_ = 0;
    std::exception_ptr err_;
};

// Ownership and teardown. Every handle of a context has an owning type
// (DevBuf, Stream, Event, PinnedBuf, unique_ptr), so ~Ctx releases nothing by
// hand: it only ends the host threads, in the order pinning thread, expander,
// packing pool, after which no thread can touch the context's memory. The
// members then go in reverse order of declaration, in two groups: first the
// streams, events and page-locked buffers (with the slots, whose events go
// before their buffers), which therefore stand at the end of the struct; then
// the device buffers and the index parts, which stand before them. A new
// member goes with its kind.
struct Ctx {
    int device = 0;
    Placement place;                      // NUMA node of the device; the context's threads run there
    int numCU = 0;
    DeviceIndex I;
    // A text of 2^32 - 2 symbols or more is indexed in parts (splitRecords):
    // part 0 is I, parts 1.. are `more`; a search runs over each part in turn
    // (swapped into I) and merges the hits (run). partRec0[p] = the global id
    // of part p's first record. exportPart selects the part the export test
    // hooks read (sahara_gpu_select_part).
    std::vector<DeviceIndex> more;
    std::vector<uint64_t> partRec0{0};
    uint32_t exportPart = 0;
    DevBuf<sahara_hit> outAll;            // multi-part: hits of the parts so far
    MergeBufs merge;                      // multi-part: sort keys of the merge by qid

    // staged inputs
    DevBuf<uint32_t> pats;                // 4-bit packed patterns, patWords per pattern (FM phase)
    DevBuf<uint4> pats3;                  // 3-bit-plane blocks, patBlocks per pattern (text phase)
    uint64_t npat = 0;
    uint32_t m = 0, patWords = 0, patBlocks = 0;
    DevBuf<uint32_t> scheme, cover, kmerStart;        // FM scheme table; text table (textTable)
    uint32_t nsearch = 0;                 // (several rounds: the most of any round, what the geometry is planned for)
    uint32_t maxErr = 0;
    // The rounds of a pass (stageSchemes). Every call but besthits has one.
    // A besthits call has one per exact-j scheme, their tables side by side in
    // scheme / cover / kmerStart: round r's begin at its schemeAt / coverAt /
    // kmerAt (words). Each batch runs the rounds in turn in its slot, a round
    // seeding only the patterns that have not reported yet (pass.cpp issueFM).
    struct Round {
        uint32_t nsearch = 0, maxErr = 0;
        size_t schemeAt = 0, coverAt = 0, kmerAt = 0;
    };
    std::vector<Round> rounds;
    bool edit = true;
    bool verify = true;
    bool locateSA = true;

    DevBuf<uint4> stack;                 // FM spill stack (stream st only)
    DevBuf<uint8_t> rawPats;              // staged pattern bytes before packing
    DevBuf<uint8_t> nibPats;              // the same, two symbols per byte as uploaded (stageIn)
    bool nibbleUpload = true;             // SAHARA_NIBBLE_UPLOAD=0: pattern bytes go up as given
    DevBuf<uint32_t> small;               // scratch counters for single-stream helpers
    DevBuf<unsigned long long> counters;  // nodes, rank nodes, lines, lf steps, digest, text nodes, tasks
    DevBuf<uint64_t> qoff, k0, k1;        // per-query row segments of a batch; locate keys
    DevBuf<uint64_t> partial;             // tile sums of the segment scan
    DevBuf<uint32_t> big, huge;           // long / huge segments
    DevBuf<char> tmp;
    DevBuf<sahara_hit> out;
    uint64_t nout = 0;
    double stageMs = 0;                   // wall time of the last stage(): H2D, pack, validation
    uint32_t hitCap = 0, taskCap = 0;
    sahara_stats stats{};

    // Streamed query upload (sahara_gpu_search, sahara_gpu_search_reads): the
    // source rows go up in chunks, each packed on the host (two symbols per
    // byte, ranks checked) into a slot of a pinned ring and copied on stream
    // stE when the first batch that needs it is issued, so that the upload of
    // later batches overlaps the search of earlier ones. ringEv[s] fires once
    // slot s's last DMA is done: the device-side unpacking waits for it, and
    // the host waits for it before packing into the slot again. The ring is
    // pinned once per context, in the background while the index loads.
    struct Upload {
        const uint8_t* src = nullptr;  // host symbols: the patterns, or the reads (rc); prepacked: 2-bit codes
        bool rc = false;               // reads: reverse complements interleaved on the device
        uint32_t bits = 4;             // 2: ACGT codes + N list, 4: nibbles, 8: bytes as given
        uint64_t rows = 0;             // source rows
        uint64_t chunk = 0;            // source rows per chunk (even: chunks start at even symbols)
        uint64_t done = 0;             // source rows enqueued
        uint64_t submitted = 0;        // chunks whose packing is posted to the pool (2 bits)
        uint32_t ahead = 6;            // chunks packed ahead of the issued ones (SAHARA_PACK_AHEAD)
        bool bad = false;              // a chunk held a byte that is no rank of this index
        double hostMs = 0;             // host time spent packing and enqueueing
        uint64_t chunks[3] = {0, 0, 0};  // chunks sent at 2 / 4 / 8 bits per symbol
        // reads that arrive two bits per symbol (sahara_gpu_search_packed):
        // chunks are copied into the ring, not packed; source symbol s of
        // the call is stream symbol sym0 + s; the N positions of the call's
        // reads are on the device (nList, relative to each chunk's first
        // whole byte), chunk j's from entry nFirst[j]
        bool prepacked = false;
        bool srcPinned = false;        // prepacked codes in page-locked memory: DMA'd from there, no copy
        uint64_t sym0 = 0;
        std::vector<uint64_t> nFirst;
    } up;
    DevBuf<uint32_t> nList;
    // the packed reads' N list last checked whole (strictly ascending): a
    // stream processed shard by shard is checked once, not once per shard
    const uint64_t* nPosChecked = nullptr;
    uint64_t nCountChecked = 0;
    static constexpr size_t kRingSlots = 8, kRingSlot = 32u << 20;  // 256 MB pinned
    // Chunks packed ahead (2-bit upload): chunk j packs into ring slot
    // j % kRingSlots on the pool's threads while the issuing thread still
    // enqueues earlier batches; uploadChunk waits for its pieces, then lists
    // the N positions and enqueues the DMA (staging.cpp packAhead).
    struct PackJob {
        uint64_t chunk = UINT64_MAX;               // in flight or finished: chunk index
        uint64_t pieces = 0, pieceSyms = 0;
        std::atomic<int> bad{0};
        std::vector<std::vector<uint32_t>> exc;    // per piece: N positions (chunk-relative symbols)
        TaskGroup group;
    } packJobs[kRingSlots];
    std::thread ringInit;                 // pins the ring (started by newCtx)
    uint64_t ringLoadNext = 0;            // uploadViaRing's next slot
    bool ringFailed = false;
    DevBuf<uint32_t> badFlag;             // device rank check of streamed chunks
    DevBuf<uint8_t> readRaw;              // streamed reads before the reverse-complement interleave
    std::unique_ptr<TaskPool> pool;       // the packing threads (hostPool)
    unsigned poolCap = 0;
    Placement packPlace;                  // the pool's CPUs when bound
    int poolNode = -2;                    // NUMA node the pool is bound to (-1: unbound)
    // The state of one call: staging starts it from Sink{} (stage,
    // stageStreamed), the entry point fills in where its hits go, and a call
    // that fails leaves it cleared (capi.cpp abandonCall).
    struct Sink {
        bool staged = false;              // patterns are staged: sahara_gpu_run may search them
        bool streaming = false;           // ... chunk by chunk during the pass (Upload)
        // where each batch's sorted hits go on stF while later batches search
        // (hit_route.h: the entry point sets it, Pass::finish asks decideBatch)
        HitRoute route = HitRoute::Device;
        bool wholeFallback = false;       // CallRoute's (Expander into a pinned sink)
        // the host sink: whole hits (PinnedWhole, Expander) or 8-B records
        // (Records; null when that call's buffer is not page-locked)
        void* host = nullptr;
        sahara_hit* hits() const { return static_cast<sahara_hit*>(host); }
        uint64_t* recs() const { return static_cast<uint64_t*>(host); }
        uint64_t cap = 0, done = 0;       // hits (records) the sink holds; those on their way into it
        bool ok = false;                  // every batch so far went into the sink
        uint64_t downJobs = 0;            // batches handed to the expander this call
        // --max_hits n applied per batch on the device (single-part indexes;
        // limitBatch), 0: off
        uint32_t limitN = 0;
    } sk;
    uint64_t lastHits = 0;                // hits of the previous sahara_gpu_search (sink size estimate)
    // compact download into the sink (Expander): device records of the
    // pass, their pinned host staging, one event per batch's download
    // (batch b's records land in slot b % kDownSlots of a pinned ring,
    // pinned with the upload ring; the slot is reused once batch b is expanded)
    DevBuf<uint64_t> outC;
    static constexpr size_t kDownSlots = 3, kDownSlot = 64u << 20;  // 8M records per batch
    std::unique_ptr<Expander> expander;
    // sahara_gpu_search_reads_compact: each batch's hits as 8-B records in
    // HBM (outRecs, at the batch's place among the call's hits) and copied by a
    // copy engine on stF into the pinned host buffer sk.recs() (sk.cap records); per
    // batch its first qid and one past its last record (the blocks of
    // sahara_hit_blocks). (Written by the kernel straight into the sink over
    // PCIe, the records held CU slots beside the text phase: C3 592M against
    // 632M reads/s with the copy engine, profiles/r03_pcie_compact_dma.txt.)
    // A batch whose sink takes compact records is sorted straight into them
    // (pass.cpp finish: batchDirect), and `out` holds nothing of it until a
    // reader of the whole hits asks (wholeHits below); the Expander's
    // batches go through outRecs in the same way.
    DevBuf<uint64_t> outRecs;
    std::vector<uint64_t> batchQ0, batchEnd;
    std::vector<uint8_t> batchDirect;     // per batch: its hits are in outRecs only
    bool outStale = false;                // some batch is: `out` lacks its hits
    // The last pass's hits as whole records, device-resident: `out`, after
    // the batches that were sorted into compact records are expanded into it
    // (once, off any timed path: sahara_gpu_fetch, _digest, _copy_hits and the
    // copy-out of a sink that was too small).
    const sahara_hit* wholeHits();
    void reserveRecs(size_t n) {          // (outRecs may be all there is of the last call's hits)
        if (n > outRecs.cap) wholeHits();
        outRecs.reserve(n);
    }
    std::vector<uint64_t> recStartsEnd;   // record starts + the text length (sahara_hit_blocks.rec_starts)
    // The stages a batch's sorted whole hits go through before they leave the
    // device (pass_plan.h Stage; pass.cpp Pass::stages). stageScratch: where
    // each gathers the records it leaves (search.h BatchView::scratch).
    DevBuf<sahara_hit> stageScratch;
    LimitBufs limit;                      // --max_hits (sk.limitN; hits.hip limitBatch)
    // The stages' figures of the last search call, summed over its batches,
    // parts and host besthits passes; together, so that a call clears them
    // and an overflow re-run restores them as one value (pass.cpp run, runOne).
    struct StageStats {
        sahara_loci_stats loci{};
        sahara_rescue_stats rescue{};
        sahara_pairs_stats pairs{};
        double linkMs = 0;  // the pair stage's two link kernels, a part of pairs.kernel_ms
        // by Stage, what every stage keeps alike: the batches it ran on and its
        // HIP-event time (--max_hits keeps no figures: nulls)
        struct Figures {
            uint64_t* batches;
            double* kernelMs;
        };
        Figures figures(uint32_t stage) {
            const Figures f[kStages] = {{&loci.batches, &loci.kernel_ms}, {&rescue.batches, &rescue.kernel_ms},
                                        {&pairs.batches, &pairs.kernel_ms}, {nullptr, nullptr}};
            return f[stage];
        }
    } stageStats;
    // The loci stage (docs/semantics.md "Loci"; loci.hip): a setting of the
    // context, not of a call (sahara_gpu_set_loci): when on, every batch of
    // every pass cuts its whole hits to one record per locus right after the
    // sort.
    struct Loci {
        bool on = false;
        uint32_t window = 0;
        LociBufs bufs;
    } loci;
    // The pair stage (docs/semantics.md "Pairs"; pairs.hip): a setting of the
    // context as well (sahara_gpu_set_pairs): when on, every batch of every
    // pass, cut at multiples of four patterns, keeps only its hits with a
    // concordant mate, after the loci stage and before --max_hits.
    struct Pairs {
        bool on = false;
        uint32_t minFrag = 0, maxFrag = 0;
        PairsBufs bufs;
        // Best mode (docs/semantics.md "Best pairs"; sahara_gpu_set_best_pairs):
        // the stage keeps each pair's least-error placements within delta.
        // summary: the last call's per-pair records in pinned host memory,
        // sized per call (pass.cpp run); summaryOn: that call ran in best mode.
        bool best = false;
        uint32_t delta = 0;
        PinnedBuf<sahara_pair_summary> summary;
        uint64_t summaryPairs = 0;
        bool summaryOn = false;
        // Links (docs/semantics.md "Pair links"; sahara_gpu_set_pair_links):
        // in best mode the stage also writes one link per hit it keeps.
        // linkBuf: the last call's, in pinned host memory, hit 0 first, grown
        // per batch; linksOn: that call wrote them, linkCount of them.
        bool links = false;
        PinnedBuf<sahara_pair_link> linkBuf;
        uint64_t linkCount = 0;
        bool linksOn = false;
    } pairs;
    // The mate rescue (docs/semantics.md "Mate rescue"; rescue.hip): a setting
    // of the context too (sahara_gpu_set_rescue), which needs the pair stage
    // on: every batch gets the windows of its hits without a mate scanned for
    // the partner's pattern within maxErr errors, after the loci stage and
    // before the pair stage.
    struct Rescue {
        bool on = false;
        uint32_t maxErr = 0, maxAnchors = 0;
        RescueBufs bufs;
    } rescue;
    // SAHARA_TIMING=2: host-side marks of one call (ms since its start, what)
    bool traceOn = false;
    std::chrono::steady_clock::time_point traceT0;
    std::mutex traceMu;
    std::vector<std::pair<double, std::string>> trace;
    void mark(const char* what, uint64_t i) {
        if (!traceOn) return;
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - traceT0).count();
        std::lock_guard<std::mutex> g(traceMu);
        trace.emplace_back(t, std::string(what) + " " + std::to_string(i));
    }

    // work buffers. Batches rotate over kSlots slots so that seeds and the FM
    // phase run batches ahead (streams `stD`, `st`) of the text phase (stream
    // `stB`), while earlier batches run their locate and sort (stream `stC`).
    static constexpr int kSlots = 5;
    struct Slot {
        DevBuf<uint4> hits, tasks, seeds;  // seeds: starting cursors (kSeedItems -> kSearchFM)
        DevBuf<uint32_t> seedItem;
        DevBuf<uint32_t> qcnt, rank;      // rows ranked at emission: per-query row counts (zero between
                                          // batches), per hit slot its first row's place in its segment
        DevBuf<uint32_t> small;           // the slot's counters, by SlotWord (search.h)
        DevBuf<uint32_t> queues;          // striped work counters, three queues at QueueAt (search.h)
        // kernel spans, each recorded on the kernel's own stream right around
        // its launch(es): seeds fmStart..seedDone (sD), FM fmBegin..fmDone
        // (sA), text textStart..textDone (sB); seedDone0: the batch's first
        // seed tasks are written
        Event fmStart, seedDone, seedDone0, seedMid, fmBegin, fmDone, textStart, textDone, free;
        // the first batch of an early pass launches its text phase twice:
        // textStart..textMid0, then textMid1..textDone (not the wait between)
        Event textMid0, textMid1;
        bool twoText = false;
        bool seedsInParts = false;        // seeds in parts: fmStart..seedDone0, then Ctx::partEv's pairs
        uint32_t seedParts = 0;           // (the later parts: Ctx::partEv[2 i], [2 i + 1] around part i)
        // several rounds per batch: the last round records the events above
        // (so the finisher waits for textDone as ever), round r before it
        // earlier[r] (made by runPass before the pass's threads start)
        struct RoundEvents {
            Event fmStart{hipEventDefault}, seedDone{hipEventDefault}, fmBegin{hipEventDefault},
                fmDone{hipEventDefault}, textStart{hipEventDefault}, textDone{hipEventDefault};
        };
        std::vector<RoundEvents> earlier;
    } slot[kSlots];

    // sahara_gpu_align[_packed_compact]: the call's patterns, whole, as
    // 3-bit-plane blocks (one spare block after the last: align.h), with the
    // staging they are packed from (rank bytes; 2-bit codes, their N list and
    // the 4-bit twin kPackFrom2 writes beside the blocks); one chunk of hit
    // records going up and of alignment records coming down; a compact call's
    // blocks (block_end, then block_qid0)
    struct Align {
        DevBuf<uint4> pats3;
        DevBuf<uint8_t> raw;
        DevBuf<uint32_t> nList, pats4;
        DevBuf<char> in;
        DevBuf<sahara_alignment> out;
        DevBuf<uint64_t> blocks;
        sahara_align_stats stats{};
    } align;

    // Streams, events and page-locked memory: declared last, released first
    // (the rule at the top of Ctx).
    Stream st, stB, stC, stD;  // FM phase and single-stream work; text, locate / sort, seeds
    Stream stE, stF;           // pattern upload; hit download (sink)
    Event outCopied[2];        // capi.cpp copyOut: a staging chunk's DMA is done
    // a batch's locate chain on stC (pass.cpp finish): its start, locate and
    // sort + decode done (timing), the batch's totals and its locate flags
    // in the pinned record, its compact records made
    Event locStart, locDone, sortDone, totalsDown, flagsDown, recsMade;
    // around each of a batch's stages on stC, by Stage (their stats' kernel_ms;
    // --max_hits keeps no figures and records none)
    Event stageStart[kStages], stageDone[kStages];
    // the finisher's waits in a streamed call, recorded in place of totalsDown
    // and beside flagsDown: blocking-sync events, so that it sleeps instead of
    // spinning a CPU that the packing threads need (a 16-CPU quota on the GPU box)
    Event totalsDownSleep, flagsDownSleep;
    std::vector<Event> partEv;  // around the first batch's later seed launches (created on demand)
    Event ringEv[kRingSlots];
    std::vector<Event> downEv;
    // SAHARA_TIMING=2: timing events around each chunk's DMA (bytes, events)
    std::vector<std::pair<uint64_t, std::pair<Event, Event>>> dmaEv;
    size_t dmaUsed = 0;
    PinnedBuf<BatchRecord> pinned;        // per batch: host copies of its slot's counters and totals
    // two pinned staging chunks for handing hits to pageable host memory: the
    // DMA of one chunk overlaps the host copy out of the other (copyOut)
    static constexpr size_t kOutChunk = 32u << 20;
    PinnedBuf<char> outStage[2];
    PinnedBuf<uint8_t> nibHost;           // the packed patterns on their way up (stage)
    PinnedBuf<uint8_t> ring;              // the upload ring (pinned by ringInit)
    PinnedBuf<uint64_t> downRing;         // the compact download's ring (pinned with it)

    // Host threads end here, before any member goes: the pinning thread
    // (it assigns ring and downRing), the expander (it reads downRing and
    // waits on downEv), the packing pool (it writes into ring).
    ~Ctx() {
        if (ringInit.joinable()) ringInit.join();
        expander.reset();
        pool.reset();
    }
};

// f() when the scope ends, on every way out unless dismissed
template <typename F>
struct ScopeExit {
    explicit ScopeExit(F g) : f(std::move(g)) {}
    ~ScopeExit() {
        if (armed) f();
    }
    void dismiss() { armed = false; }
    F f;
    bool armed = true;
};

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
    } catch (...) {
        g_err = "unknown error";
    }
    return -1;
}

bool hitLess(const sahara_hit& a, const sahara_hit& b);
void limitHits(std::vector<sahara_hit>& v, uint32_t n);
void handOver(const std::vector<sahara_hit>& v, sahara_hit** hits, uint64_t* n_hits);
// capi_ctx.cpp: context lifecycle and placement
Ctx* newCtx(int device);
unsigned hostThreads(const Ctx* c, unsigned cap);
Ctx* ctxOf(void* p);
TaskPool& hostPool(Ctx* c);
Placement placementOfNode(int node);
// host bytes -> device through the pinned upload ring, copied into it by the
// pool's threads (an index image's arrays: staging.cpp)
void uploadViaRing(Ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
// every pack job posted by the streamed upload is finished (the caller's
// source buffer is no longer read): before a new call stages, after a failed one
void drainPacking(Ctx* c);

// staging.cpp: the FM scheme table (the text phase's is text_step.h's
// textTable), the query packers, the streamed upload
void packSchemeTable(const uint32_t* pi, const uint32_t* l, const uint32_t* u, uint32_t ns, uint32_t m,
                     std::vector<uint32_t>& out, uint32_t& maxErr);
bool hostHasAvx2();
bool hostHasAvx512();
uint64_t pack2Best(const uint8_t* in, uint8_t* out, uint64_t count, uint32_t sigma, uint64_t base,
                   std::vector<uint32_t>& exc);
uint64_t pack2Avx512(const uint8_t* in, uint8_t* out, uint64_t count, uint32_t sigma, uint64_t base,
                     std::vector<uint32_t>& exc);
uint64_t pack2Scalar(const uint8_t* in, uint8_t* out, uint64_t count, uint32_t sigma, uint64_t base,
                     std::vector<uint32_t>& exc);
uint64_t pack2Avx2(const uint8_t* in, uint8_t* out, uint64_t count, uint32_t sigma, uint64_t base,
                   std::vector<uint32_t>& exc);
void uploadChunk(Ctx* c, hipStream_t kst);
void ensureUploaded(Ctx* c, uint64_t patEnd, hipStream_t kst);
// (the scheme half of staging: nrounds schemes back to back, ns[r] rows each: Ctx::rounds)
void stageSchemes(Ctx* c, uint64_t npat, uint32_t m, const uint32_t* pi, const uint32_t* l, const uint32_t* u,
                  const uint32_t* ns, uint32_t nrounds, int edit);
// reads given two bits per symbol (sahara_gpu_search_packed[_compact])
struct PackedReads {
    uint64_t sym0;          // stream position of the first read's first symbol
    const uint64_t* nPos;   // stream positions of N, ascending (any outside the reads are ignored)
    uint64_t nCount;
};
// (nrounds schemes back to back, ns[r] rows each: one, or the rounds of a besthits call)
void stageStreamed(Ctx* c, const uint8_t* src, uint64_t rows, bool rc, uint64_t npat, uint32_t m,
                   const uint32_t* pi, const uint32_t* l, const uint32_t* u, const uint32_t* ns, uint32_t nrounds,
                   int edit, const PackedReads* packed = nullptr);
void stage(Ctx* c, const uint8_t* ranks, uint64_t npat, uint32_t m, const uint32_t* pi, const uint32_t* l,
           const uint32_t* u, const uint32_t* ns, uint32_t nrounds, int edit);

// capi.cpp: host buffers handed to the caller, and what the alignment calls
// (capi_align.cpp) share with the search calls
// a host buffer on its way to the caller, freed by freeHits (allocHits, allocPinned) or std::free
using HostBuf = std::unique_ptr<void, void (*)(void*)>;
void* allocPinned(size_t bytes, bool* pinned, size_t* capBytes, bool mayPin, bool always = false);
void freeHits(void* p);
void copyOut(Ctx* c, void* dst, const void* src, size_t bytes);
// The query list of a reads call: n_reads reads, interleaved with their
// reverse complements (reverse) and cut to `limit` patterns (--limit_queries
// cuts the interleaved list, search.cpp:125-127); rows: the reads it takes.
struct ReadRows {
    uint64_t npat, rows;
};
ReadRows readRows(int reverse, uint64_t n_reads, uint64_t limit);

// pass.cpp: one pass over the staged patterns (every part of the index)
DeviceIndex& partOf(Ctx* c, uint32_t p);
void run(Ctx* c, bool count);
// with the pair stage on: what a call of npat patterns of length len must satisfy (throws otherwise);
// the entry points ask before they stage anything, run() asks again for sahara_gpu_run
void checkPairsCall(const Ctx* c, uint64_t npat, uint32_t len);
void runOne(Ctx* c, bool count);
void runPass(Ctx* c, bool count, bool serial, sahara_stats& S, bool& overflow);
void growCap(uint32_t& cap, uint32_t seen);
// the buffers of a pass with batches of maxBatch patterns, as the pass sizes
// them (sahara_gpu_prepare makes them ahead of the first call)
void initWorkCaps(Ctx* c, uint64_t maxBatch, const PassKnobs& k);
void reserveSlot(Ctx* c, Ctx::Slot& sl);
void reserveLocate(Ctx* c, uint64_t maxBatch, uint64_t nslots);

}  // namespace sahara
