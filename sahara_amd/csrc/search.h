// search.h — host-side launch interface of the search / locate kernels, grouped
// by the unit that defines them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sahara_hip.h"
#include "device_index.h"

namespace sahara {

struct SearchArgs {
    const OccLine* occF;
    const OccLine* occR;
    uint32_t C[8];
    uint32_t n;              // text length incl. delimiters (root interval length)
    const uint32_t* pats;    // npat * patWords 4-bit packed pattern words
    uint32_t patWords;
    uint32_t m;
    uint32_t nsearch;
    uint32_t nitems;         // npat * nsearch
    const uint4* seeds;      // starting cursors (kSeedItems), *seedCount of them
    const uint32_t* seedItem;  // their items (pattern * nsearch + search)
    const uint32_t* seedCount;
    const uint32_t* scheme;  // nsearch * m packed entries (packScheme)
    uint32_t* work;          // item counter
    uint4* stack;            // spilled DFS levels beyond the LDS part, [depth][grid thread]
    uint32_t stackCap;       // most entries a lane's stack holds (the DFS bound)
    uint32_t stackLevels;    // levels per lane, a ring (>= stackCap: work stealing moves a stack's bottom up)
    uint32_t stealAt;        // once the seed queue is dry: idle lanes take the bottom stack entry of a busy
                             // lane of their wave once this many are idle (0: off)
    uint4* hits;             // (qid, lb, len, e) or (qid, text pos, 1, e | kPosKnown)
    uint32_t hitCap;
    uint32_t* hitCount;      // reserved slots (waves reserve ranges; unused slots have len 0)
    uint32_t* filled;        // records actually written
    uint32_t* flags;         // Flag bits
    unsigned long long* counters;  // by Counter
    uint4* tasks;            // text tasks (fm_step.h: taskRecord)
    uint32_t taskCap;
    uint32_t* taskCount;
    uint32_t split;          // intervals of <= split rows go to the text phase (0: never)
    uint32_t ldsDepth;       // DFS levels kept in LDS (after the scheme table; the rest spill to HBM)
    // rows ranked where the hits are written: rank[slot] = the hit's first
    // row in its query's segment, qcnt[qid] += len (the batch's per-query row
    // counts, zero on entry; the locate chain's scan reads and clears them)
    uint32_t* qcnt;
    uint32_t* rank;
};

struct SeedArgs {
    const uint32_t* pats;
    uint32_t patWords;
    uint32_t nsearch;
    uint32_t itemBegin;         // items [itemBegin, nitems) of the batch (a batch's seeds in parts)
    uint32_t nitems;
    uint32_t n;
    const uint4* kmer;          // k-mer table (DeviceIndex::kmer), nullptr = start every item at the root
    uint32_t kmerK;
    uint32_t kmerPos;           // the table holds SA[lb] of single-row entries: their tasks carry text positions
    const uint32_t* kmerStart;  // per search: pattern offset of its error-free first kmerK steps, ~0u = n/a
    uint4* seeds;
    uint32_t* seedItem;
    uint32_t* seedCount;
    // a seed whose k-mer occurs once is already a text task: written straight
    // to the task list (the FM kernel's record format) instead of the seeds
    uint32_t m;
    uint32_t toText;            // 1: convert single-row seeds (the text phase runs, split >= 1)
    uint4* tasks;
    uint32_t taskCap;
    uint32_t* taskCount;
    uint32_t* flags;            // kFlagTasks: task buffer too small
    unsigned long long* counters;  // count mode: text tasks (kCtTextTasks), else nullptr
    // besthits rounds (pass.cpp): the batch's per-pattern row counts so far
    // (the slot's qcnt), nullptr = none. An item whose pattern has reported
    // (skip[pid] != 0) is dropped before its k-mer lookup: no seed, no task;
    // count mode counts the dropped items (kCtBestSkipped).
    const uint32_t* skip;
};

// Layouts that the host code (pass.cpp) and the kernels share, each defined
// once here.
// the words of a slot's counters (Ctx::Slot::small); kBatchTotals copies all
// kSlotWords of them into the batch's record
enum SlotWord : uint32_t {
    kSwRoundTasks = 0,  // taskCount when the round began (kRoundReset): the round's text launch starts there
    kSwHitCount = 1, kSwFlags = 2, kSwFilled = 3, kSwTaskCount = 4,
    kSwSeedTasks = 5,  // taskCount once the batch's seed tasks are all written (an early text launch's end)
    kSwSeedCount = 6, kSlotWords = 8
};
// the bits of a flags word (a slot's kSwFlags; the locate chain's own word)
enum Flag : uint32_t {
    kFlagStack = 1,      // FM DFS stack bound violated
    kFlagHits = 2,       // hit buffer too small
    kFlagLocate = 4,     // locate walked off the SA samples
    kFlagTasks = 8,      // task buffer too small
    kFlagTextStack = 16  // text DFS stack bound violated
};
// a slot's striped work queues (Ctx::Slot::queues), kQueueWords counter words
// each (search_device.h: kStripes * kStripeStride): the FM phase's seeds, the text
// phase's seed tasks, the tasks the FM phase appended
constexpr uint32_t kQueueWords = 256;
enum QueueAt : uint32_t { kQueueSeeds = 0, kQueueSeedTasks = kQueueWords, kQueueFmTasks = 2 * kQueueWords,
                         kQueuesWords = 3 * kQueueWords };
// One batch's record in pinned host memory (Ctx::pinned), written by
// kBatchTotals (words 0-11), kLocateFlagsOut (7), the batch's stages through BatchView::kept (12-13, one
// after the other) and pairsBatch (14-15)
struct BatchRecord {
    uint32_t slot[7];      // the slot's counters, by SlotWord
    uint32_t locateFlags;  // the locate chain's flags word (kFlagLocate)
    uint64_t rows;         // the batch's row total
    uint32_t nbig, nhuge;  // long / huge segments
    uint64_t kept;         // the word every stage reads its count back through (scanFlagsCount, limitBatch): the
                           // host has read one stage's before the next stage writes its own
    uint64_t pairs;        // pairs that keep a hit (the pair stage; read after the batch's chain)
};
static_assert(sizeof(BatchRecord) == 64 && offsetof(BatchRecord, slot) == 0 &&
              offsetof(BatchRecord, locateFlags) == 4 * 7 && offsetof(BatchRecord, rows) == 4 * kSlotWords &&
              offsetof(BatchRecord, nbig) == 4 * 10 && offsetof(BatchRecord, nhuge) == 4 * 11 &&
              offsetof(BatchRecord, kept) == 4 * 12, "BatchRecord is what kBatchTotals and the batch's stages write");

// work counters of count mode (sahara_stats; Ctx::counters)
constexpr uint32_t kCounters = 56;
enum Counter : uint32_t {
    kCtNodes = 0, kCtRankNodes = 1, kCtExtLines = 2, kCtLfSteps = 3, kCtDigest = 4, kCtTextNodes = 5,
    kCtTextTasks = 6, kCtFmIter = 7, kCtTextIter = 8, kCtTextActive = 9, kCtTextRefills = 10,
    kCtCyRefill = 11, kCtCyStep = 12, kCtCyEmit = 13,  // text-kernel cycles
    kCtCompareSteps = 14, kCtTextSteps = 15,
    kCtPosTasks = 16,  // text tasks that came with their text position (kTaskPos)
    kCtBestSkipped = 17,  // items of patterns that had reported in an earlier round (SeedArgs::skip)
    // TextBatchArgs::probe, the pass's first text launch, wall clock (10 ns):
    // per wave that saw the queue dry, its time after that and their number
    kCtDryRun = 30, kCtDryWaves = 31,
    kCtBornMin = 33, kCtBornMax = 34, kCtEndMax = 35, kCtLifeSum = 36, kCtEndMin = 37,  // wave starts / ends (minima start at ~0)
    kCtDryMin = 38, kCtDryMax = 39,  // the queue seen dry first / last
    kCtIterPre = 40, kCtActPre = 41, kCtIterPost = 42, kCtActPost = 43,  // iterations, busy lanes before / after
    kCtStolen = 45,                                                      // text nodes stolen (all launches)
    kCtWallPreRefill = 46, kCtWallPreStep = 47, kCtWallPostRefill = 48, kCtWallPostStep = 49
};
// One launch of the text phase over one batch's tasks [*taskBegin, *taskCount)
// (kSearchTextBatch)
struct TextBatchArgs {
    const uint32_t* sa;      // full SA: task records carry SA rows (unless kTaskPos, fm_step.h), the kernel reads their positions
    const uint4* text3;      // text as 3-bit-plane blocks of 32 symbols (device_index.h)
    const uint4* pats3;      // the batch's patterns as 3-bit-plane blocks, patBlocks per pattern
    uint32_t patBlocks;
    uint32_t text3Bytes;     // bytes of text3 / of the batch's pats3 (buffer-load bounds; < 4 GiB)
    uint32_t pats3Bytes;
    uint32_t m;
    uint32_t nsearch;
    const uint2* table;      // nsearch * m rows (text_step.h: TextRow, textTable)
    const uint4* tasks;
    const uint32_t* taskCount;  // tasks written by the seed / FM kernels (device-side: no host round trip)
    const uint32_t* taskBegin;  // first task of this launch (device-side; nullptr: 0)
    uint32_t taskCap;
    uint32_t* work;          // the launch's striped queue counters (zero)
    uint4* hits;
    uint32_t hitCap;
    uint32_t* hitCount;
    uint32_t* filled;
    uint32_t* flags;
    unsigned long long* counters;
    uint32_t winBlocks;      // window blocks per lane (32 symbols each)
    uint32_t exactWindow;    // 1: the window starts at its first symbol (funnel-shifted copy), else block-aligned
    uint32_t stackCap;       // text DFS stack entries per lane
    uint32_t tableWords;     // LDS words before the lane slots: max(2 * nsearch * m, kTextTableMin)
    uint32_t steps;          // node expansions per lane between wave-level bookkeeping
    uint32_t refillAt;       // refill idle lanes once this many are idle
    uint32_t stealAt;        // once the task queue is dry: idle lanes take the bottom stack entry of a busy
                             // lane of their wave (with its window and pattern) once this many are idle (0: off)
    uint32_t* qcnt;          // as SearchArgs: rows ranked where the hits are written (the FM phase's counts)
    uint32_t* rank;
    uint32_t probe;          // (count mode) wave lives on the wall clock into counters kCtDryRun.. ...
    uint32_t isFirst;        // ... for the pass's first launch only
};

struct LocateArgs {
    const uint4* hits;
    uint64_t nhits;
    const uint64_t* qoff;          // per-query row segments (querySegments)
    const uint32_t* rank;          // per cursor: slot of its first row in the segment (querySegments)
    const OccLine* occF;
    uint32_t C[8];
    const uint32_t* samples;
    uint32_t rate;
    uint64_t* keys;
    uint32_t* flags;
    unsigned long long* counters;  // lf steps
    const uint32_t* sa;            // full SA: locate = one read (when useSA)
    uint32_t useSA;
};

// ---- search_fm.hip: the seeds and the FM phase of one batch (kSeedItems, kSearchFM)
int searchBlocksPerCU(uint32_t sigma, bool edit, size_t lds);
void launchSeeds(const SeedArgs& a, uint32_t sigma, uint32_t blocks, hipStream_t st);
void launchSearch(const SearchArgs& a, uint32_t sigma, bool edit, bool count, uint32_t blocks, size_t lds,
                  hipStream_t st);

// ---- search_text.hip: the text phase of one batch (kSearchTextBatch): the compiled
// shape that a geometry runs as, that variant's occupancy, its launch
int textShapeOf(uint32_t winBlocks, uint32_t patBlocks, bool exactWindow);
int textBlocksPerCU(bool edit, bool count, int shape, size_t lds);
void launchTextBatch(const TextBatchArgs& a, bool edit, bool count, uint32_t blocks, size_t lds, hipStream_t st);

// ---- locate_sort.hip: locate + canonical order, per batch: querySegments
// (rows per query -> segments; long segments listed in big, their count in
// *nbig, read back by the host), launchLocate (keys into the segments),
// sortDecode (short segments in registers, medium across a wave, long in LDS,
// huge by segmented radix sort).
uint32_t scanTiles(uint32_t nq);  // u64 partials querySegments needs
// qcnt: the batch's per-query row counts, which the search kernels add up
// as they write the hits (SearchArgs::qcnt); all zero on return
void querySegments(uint32_t* qcnt, uint32_t nq, uint64_t* qoff, uint64_t* partial, uint32_t* big, uint32_t* nbig,
                   uint32_t* huge, uint32_t* nhuge, hipStream_t st);
void launchLocate(const LocateArgs& a, bool count, hipStream_t st);
// the locate chain's flags word into pinned host memory (BatchRecord::locateFlags); zero afterwards
void launchLocateFlagsOut(uint32_t* flags, uint32_t* out, hipStream_t st);
size_t bigSortTempBytes(uint64_t rows, uint32_t nbig);
// long segments (> 64 rows, listed in big) are sorted in LDS, huge ones
// (> 2048, listed in huge) by the segmented radix sort
void sortDecode(uint64_t* k0, uint64_t* k1, uint64_t rows, const uint64_t* qoff, uint32_t nq, const uint32_t* big,
                uint32_t nbig, const uint32_t* huge, uint32_t nhuge, uint64_t qidBase, const uint64_t* starts,
                uint32_t nrec, sahara_hit* out, void* tmp, size_t tmpBytes, hipStream_t st);
// the same sort with the hits written as compact records (launchCompactHits'
// form, qid relative to the batch): the sorted keys with the batch-local
// query in front, so no record starts are needed; nq < 2^28
void sortCompact(uint64_t* k0, uint64_t* k1, uint64_t rows, const uint64_t* qoff, uint32_t nq, const uint32_t* big,
                 uint32_t nbig, const uint32_t* huge, uint32_t nhuge, uint64_t* out, void* tmp, size_t tmpBytes,
                 hipStream_t st);
// a batch's totals into pinned host memory in one launch: the first 12 words
// of its BatchRecord (the slot's counters, the row total, the long / huge
// segment counts), and the slot reset: small, queues (the slot's counters and
// queue words) and segCounts are zero afterwards
void launchBatchTotals(uint32_t* small, uint32_t* queues, const uint64_t* rowTotal, uint32_t* segCounts, uint32_t* out,
                       hipStream_t st);
// Between two rounds of a batch (besthits, pass.cpp): what a round consumes in
// the slot is reset: the seed count and the queue words are zero afterwards,
// and kSwRoundTasks holds the task count so far, where the next round's text
// launch begins. The hit count, filled, the flags, the task count (and qcnt,
// rank) carry over.
void launchRoundReset(uint32_t* small, uint32_t* queues, hipStream_t st);

// ---- patterns.hip: query symbols into the search's two pattern forms
void launchPackPatterns(const uint8_t* src, uint64_t npat, uint32_t m, uint32_t patWords, uint32_t sigma,
                        uint32_t* dst, uint32_t* bad, hipStream_t st);
void launchPackPatterns3(const uint8_t* src, uint64_t npat, uint32_t m, uint32_t patBlocks, uint4* dst,
                         hipStream_t st);
// n symbols, two per byte of nib (low nibble first) -> one per byte of dst
void launchUnpackNibbles(const uint8_t* nib, uint8_t* dst, uint64_t n, hipStream_t st);
// a streamed chunk of 2-bit codes (read r0's first symbol at symbol `so` of
// src, 0..3) straight into both pattern forms of the patterns [p0, p1)
void launchPackFrom2(const uint8_t* src, uint32_t so, const uint32_t* exc, uint32_t nExc, uint64_t r0, uint64_t p0,
                     uint64_t p1, uint32_t m, bool rc, uint32_t sigma, uint32_t patWords, uint32_t patBlocks,
                     uint32_t* pats, uint4* pats3, hipStream_t st);
// reads [r0, r1) (m bytes each) -> patterns [2 r0, min(2 r1, pEnd)): read, reverse complement, ...
void launchInterleaveRC(const uint8_t* reads, uint64_t r0, uint64_t r1, uint32_t m, uint32_t sigma, uint64_t pEnd,
                        uint8_t* pats, hipStream_t st);

// ---- hits.hip: a batch's hit records after the sort
void launchDigest(const sahara_hit* h, uint64_t n, unsigned long long* out, hipStream_t st);
void launchCopyHits(const sahara_hit* h, uint64_t n, uint64_t qidOffset, sahara_hit* dst, hipStream_t st);
void launchOffsetSeq(const sahara_hit* in, uint64_t n, uint64_t rec0, sahara_hit* out, hipStream_t st);
// key / index buffers of the multi-part merge (kept by the context)
struct MergeBufs {
    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> v0, v1;
};
void sortHitsByQid(const sahara_hit* in, uint64_t n, uint64_t nqid, sahara_hit* out, MergeBufs& B, DevBuf<char>& tmp,
                   hipStream_t st);
void launchCompactHits(const sahara_hit* h, uint64_t n, uint64_t qidBase, const uint64_t* starts, uint64_t* out,
                       hipStream_t st, uint32_t maxBlocks = 8192);
// compact records of one batch (first qid qidBase) back into whole hits
void launchExpandRecs(const uint64_t* recs, uint64_t n, uint64_t qidBase, const uint64_t* starts, uint32_t nrec,
                      sahara_hit* out, hipStream_t st);

// ---- The stages between a batch's sort and its sink, in pass_plan.h's order (loci.hip, rescue.hip,
// pairs.hip, limitBatch in hits.hip). Each works in place on one view of the batch, is host-synchronous
// (a count comes back through the view's pinned word and sizes what follows) and leaves the view's records
// and count as the next stage, or the sink, takes them.
struct BatchView {
    sahara_hit* hits;             // the batch's whole hits, canonical order ...
    uint64_t rows;                // ... and their count: both are what the last stage left
    uint64_t* qoff;               // their per-query segments (nq + 1 offsets): current whenever a stage starts
    uint32_t nq;                  // (pass_plan.h, the segments rule)
    uint64_t q0;                  // the batch's first qid
    DevBuf<sahara_hit>& scratch;  // where a stage gathers the records it leaves (replaceBatch copies them back)
    DevBuf<char>& tmp;            // rocPRIM's temporary storage
    uint64_t* kept;               // 8 B of pinned host memory for the count a stage reads back (BatchRecord::kept)
    hipStream_t st;
    bool later;                   // a later stage runs on this batch (laterStage): the caller sets it per stage
};
// hits.hip. The end of a stage that changed the records: the n it left in v.scratch go back over the batch
// and are its rows; the segments are written again for them iff v.later (kLociSegments: one binary search
// per query). The one place that does either.
void replaceBatch(BatchView& v, uint64_t n);
// hits.hip. num = the inclusive sum of the v.rows flags (v.rows != 0); returns num[rows - 1], the flags
// set, read back through v.kept after a sync of v.st (the stage's one host round trip)
uint64_t scanFlagsCount(uint32_t* flag, uint32_t* num, BatchView& v);

// loci.hip: the batch cut to one record per locus (docs/semantics.md "Loci")
struct LociBufs {
    DevBuf<uint32_t> flag, num;  // per record: starts a locus; its locus + 1 (the flags' inclusive sum)
    DevBuf<unsigned long long> best;  // per locus: the least (err, index) key
};
void lociBatch(BatchView& v, uint32_t window, LociBufs& B);

// rescue.hip: the mates that did not map, looked for beside the hits without one (docs/semantics.md
// "Mate rescue")
struct RescueBufs {
    DevBuf<uint32_t> flag, num, anchors;     // per record: has a mate, then is an anchor; the anchor flags'
                                             // inclusive sum (the cap); the anchors' indices
    DevBuf<sahara_hit> found, sorted;        // per anchor: its rescued record or a sentinel; sorted, then distinct
    DevBuf<unsigned long long> words;        // kRescueWords counters
    PinnedBuf<unsigned long long> host;      // ... as the host reads them
};
struct RescueIn {
    uint32_t len, minFrag, maxFrag;          // the pair rule's window (pairs_core.h pairDist)
    uint32_t maxErr, maxAnchors;             // K; A (0: no cap)
    bool edit;
    const uint64_t* recStarts;               // the part's records and text
    uint32_t nrec;
    uint64_t textLen;
    const uint4* text3;
    const uint4* pats3;                      // the batch's patterns (qid v.q0 first), patBlocks blocks each
    uint32_t patBlocks;
};
// The stage in two host-synchronous halves, so that the caller can grow the batch's buffer between them
// (and point v.hits at it again): rescueFind scans the batch's anchors, leaves the distinct rescued records
// in B.found, returns how many they are and adds its counts to `total`; rescueMerge merges those r records
// into the batch, whose buffer has room for v.rows + r.
uint64_t rescueFind(const BatchView& v, const RescueIn& in, RescueBufs& B, sahara_rescue_stats& total);
void rescueMerge(BatchView& v, uint64_t r, RescueBufs& B);

// pairs.hip: the batch cut to the hits with a concordant mate (docs/semantics.md "Pairs")
struct PairsBufs {
    DevBuf<uint32_t> flag, num;         // per record: has a mate; the flags' inclusive sum
    DevBuf<unsigned long long> pairs;   // one word: the pairs that keep a hit
    // best mode (docs/semantics.md "Best pairs"):
    DevBuf<uint8_t> err8, blk, score;   // per record: its err; per aligned 64 records: their least err; per record: m
    DevBuf<uint32_t> best;              // per pair of the batch: s1, then (a second array behind it) next
    DevBuf<sahara_pair_summary> sum;    // per pair of the batch: its summary, copied to the host per batch
    // links (docs/semantics.md "Pair links"):
    DevBuf<uint32_t> mate, ties;        // per kept record: its mate's row; per pair: its even, then odd records with m == s1
    DevBuf<unsigned long long> key;     // per pair: the least primary key (pair_links_core.h)
    DevBuf<sahara_pair_link> link;      // per record that leaves: its link, copied to the host per batch
    Event linkStart, linkDone;          // around the two link kernels of the last batch ...
    bool linkTimed = false;             // ... if they ran on it (a batch that keeps nothing runs none)
};
// The call's links in pinned host memory, hit 0 of the call first: a batch's go to buf[at ..), and buf
// grows to hold them with what lies before `at` kept (the earlier batches')
struct PairLinksOut {
    PinnedBuf<sahara_pair_link>* buf;
    uint64_t at;
};
// best mode of the pair stage: the slack, and the call's pair summaries in pinned host memory (pair 0 of the
// call first; a batch writes its pairs' from q0 / 4 on)
struct BestPairsIn {
    uint32_t delta;
    sahara_pair_summary* summary;
    const PairLinksOut* links;  // nullptr: no links
};
// *hostPairs (pinned) gets the pairs with a kept hit once v.st has passed the call; best: nullptr = off
void pairsBatch(BatchView& v, uint32_t len, uint32_t minFrag, uint32_t maxFrag, PairsBufs& B, uint64_t* hostPairs,
                const BestPairsIn* best);
// flag[i] = record i of the batch has a concordant mate in it, searched for within the partner query's
// segment (the pair stage's first step, and the rescue's)
void launchPairFlags(const BatchView& v, uint64_t dmin, uint64_t dmax, uint32_t* flag);

// hits.hip: --max_hits n, the batch's queries cut to their n best positions
struct LimitBufs {
    DevBuf<uint32_t> cnt;   // per query: the records it keeps
    DevBuf<uint64_t> off;   // ... their exclusive sum
};
void limitBatch(BatchView& v, uint32_t n, LimitBufs& B);

}  // namespace sahara
