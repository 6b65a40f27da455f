// Stand-alone check of hit_route.h (no HIP): the route of a call for every
// combination of its inputs, and the decision for one batch on every route on
// each side of every boundary, against values written out by hand and against
// a restatement of the flag logic that Pass::finish and Pass::sinkBatch held
// separately before the route was a value. tests/test_hit_route.py builds it
// under the address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../sahara_amd/csrc/hit_route.h"

using namespace sahara;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const char* name(HitRoute r) {
    switch (r) {
    case HitRoute::Device: return "Device";
    case HitRoute::PinnedWhole: return "PinnedWhole";
    case HitRoute::Expander: return "Expander";
    case HitRoute::Records: return "Records";
    }
    return "?";
}

constexpr uint64_t kSlot = 64u << 20;  // Ctx::kDownSlot: 8M records
constexpr uint64_t kQ = 1ull << 28;    // queries a compact record can tell apart

// ---- the call's route ------------------------------------------------------

static void checkCallRoute() {
    struct Row {
        bool pinned, compactOk, full, compact;
        HitRoute route;
        bool wholeFallback;
    };
    // pinned, compact possible, SAHARA_FULL_DOWNLOAD, SAHARA_COMPACT_DOWNLOAD
    const Row rows[] = {
        // pageable, no compact download possible: no sink at all
        {false, false, false, false, HitRoute::Device, false},
        {false, false, false, true, HitRoute::Device, false},
        {false, false, true, false, HitRoute::Device, false},
        {false, false, true, true, HitRoute::Device, false},
        // pageable, compact possible: the Expander unless the full download is forced
        {false, true, false, false, HitRoute::Expander, false},
        {false, true, false, true, HitRoute::Expander, false},
        {false, true, true, false, HitRoute::Device, false},
        {false, true, true, true, HitRoute::Device, false},
        // pinned, no compact download possible: whole, whatever is forced
        {true, false, false, false, HitRoute::PinnedWhole, false},
        {true, false, false, true, HitRoute::PinnedWhole, false},
        {true, false, true, false, HitRoute::PinnedWhole, false},
        {true, false, true, true, HitRoute::PinnedWhole, false},
        // pinned, compact possible: whole unless the compact download is forced
        // (and the full one is not); then whole DMA stays the per-batch fallback
        {true, true, false, false, HitRoute::PinnedWhole, false},
        {true, true, false, true, HitRoute::Expander, true},
        {true, true, true, false, HitRoute::PinnedWhole, false},
        {true, true, true, true, HitRoute::PinnedWhole, false},
    };
    for (const Row& r : rows) {
        const CallRoute got = callRoute(r.pinned, r.compactOk, r.full, r.compact);
        if (got.route != r.route || got.wholeFallback != r.wholeFallback) {
            std::fprintf(stderr, "callRoute(%d, %d, %d, %d) = %s/%d, expected %s/%d\n", r.pinned, r.compactOk, r.full,
                         r.compact, name(got.route), got.wholeFallback, name(r.route), r.wholeFallback);
            ++failures;
        }
    }
    CHECK(!sinkStarts(HitRoute::Device));
    CHECK(sinkStarts(HitRoute::PinnedWhole) && sinkStarts(HitRoute::Expander) && sinkStarts(HitRoute::Records));
}

// ---- one batch, by hand ----------------------------------------------------

static BatchIn in(HitRoute route, bool wholeFallback, bool ok, uint64_t nout, uint64_t rows, uint64_t nb, uint64_t cap,
                  uint32_t limitN = 0, bool onePart = true, uint64_t slot = kSlot) {
    return {route, wholeFallback, ok, nout, rows, nb, cap, limitN, onePart, slot};
}

static void expect(int line, const BatchIn& i, bool direct, bool needRecs, BatchCopy copy, bool compactFirst, bool ok) {
    const BatchPlan d = decideBatch(i);
    if (d.direct != direct || d.needRecs != needRecs || d.copy != copy || d.compactFirst != compactFirst || d.ok != ok) {
        std::fprintf(stderr, "line %d: %s: direct %d needRecs %d copy %d compactFirst %d ok %d, expected %d %d %d %d %d\n",
                     line, name(i.route), d.direct, d.needRecs, (int)d.copy, d.compactFirst, d.ok, direct, needRecs,
                     (int)copy, compactFirst, ok);
        ++failures;
    }
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)

static void checkBatchByHand() {
    const BatchCopy None = BatchCopy::None, Recs = BatchCopy::RecordsDma, Slot = BatchCopy::ExpanderSlot,
                    Whole = BatchCopy::WholeDma;
    const HitRoute D = HitRoute::Device, P = HitRoute::PinnedWhole, E = HitRoute::Expander, R = HitRoute::Records;
    //                                                       direct needRecs copy  compactFirst ok
    // Device: whole hits on the device, nothing copied, the sink never in step
    EXPECT(in(D, false, false, 0, 10, 4, 0),                 false, false, None,  false, false);
    EXPECT(in(D, false, true, 0, 10, 4, 100),                false, false, None,  false, false);
    EXPECT(in(D, false, false, 0, 0, 4, 0),                  false, false, None,  false, false);

    // PinnedWhole: never direct; end == cap fits, cap + 1 does not
    EXPECT(in(P, false, true, 90, 10, 4, 100),               false, false, Whole, false, true);
    EXPECT(in(P, false, true, 90, 11, 4, 100),               false, false, None,  false, false);
    EXPECT(in(P, false, false, 0, 10, 4, 100),               false, false, None,  false, false);  // ok already false
    EXPECT(in(P, false, true, 90, 0, 4, 100),                false, false, None,  false, true);   // rows == 0
    EXPECT(in(P, false, true, 90, 10, kQ, 100),              false, false, Whole, false, true);   // nb is no matter
    EXPECT(in(P, false, true, 90, 10, 4, 100, 1),            false, false, Whole, false, true);   // nor limitN
    EXPECT(in(P, false, true, 0, kSlot / 8 + 1, 4, kSlot),   false, false, Whole, false, true);   // nor the slot

    // Expander, pageable sink
    EXPECT(in(E, false, true, 90, 10, 4, 100),               true,  true,  Slot,  false, true);   // end == cap
    EXPECT(in(E, false, true, 90, 11, 4, 100),               false, false, None,  false, false);  // end == cap + 1
    EXPECT(in(E, false, false, 0, 10, 4, 100),               false, false, None,  false, false);  // ok already false
    EXPECT(in(E, false, true, 90, 0, 4, 100),                false, false, None,  false, true);   // rows == 0
    EXPECT(in(E, false, true, 0, kSlot / 8, 4, kSlot),       true,  true,  Slot,  false, true);   // rows * 8 == kDownSlot
    EXPECT(in(E, false, true, 0, kSlot / 8 + 1, 4, kSlot),   false, false, None,  false, false);  // kDownSlot + 8: ends the run
    EXPECT(in(E, false, true, 0, 10, kQ - 1, 100),           true,  true,  Slot,  false, true);   // nb == 2^28 - 1
    EXPECT(in(E, false, true, 0, 10, kQ, 100),               false, false, None,  false, false);  // nb == 2^28: ends the run
    EXPECT(in(E, false, true, 0, 10, 4, 100, 1),             false, false, Slot,  true,  true);   // limitN: compacted first
    EXPECT(in(E, false, true, 0, 10, 4, 100, 0, false),      false, false, Slot,  true,  true);   // two parts (run() gives
                                                                                                   // Device before this)
    // Expander, pinned sink: whole DMA where no slot takes the batch
    EXPECT(in(E, true, true, 0, kSlot / 8, 4, kSlot),        true,  true,  Slot,  false, true);
    EXPECT(in(E, true, true, 0, kSlot / 8 + 1, 4, kSlot),    false, false, Whole, false, true);
    EXPECT(in(E, true, true, 0, 10, kQ - 1, 100),            true,  true,  Slot,  false, true);
    EXPECT(in(E, true, true, 0, 10, kQ, 100),                false, false, Whole, false, true);
    EXPECT(in(E, true, true, 90, 11, 4, 100),                false, false, None,  false, false);
    EXPECT(in(E, true, true, 90, 0, 4, 100),                 false, false, None,  false, true);

    // Records, pinned block buffer
    EXPECT(in(R, false, true, 90, 10, 4, 100),               true,  true,  Recs,  false, true);   // end == cap
    EXPECT(in(R, false, true, 90, 11, 4, 100),               true,  true,  None,  false, false);  // end == cap + 1: still direct
    EXPECT(in(R, false, false, 0, 10, 4, 100),               true,  true,  None,  false, false);  // ok already false
    EXPECT(in(R, false, true, 90, 0, 4, 100),                false, true,  None,  false, true);   // rows == 0
    EXPECT(in(R, false, true, 0, kSlot / 8 + 1, 4, kSlot),   true,  true,  Recs,  false, true);   // no slot on this route
    EXPECT(in(R, false, true, 0, 10, kQ - 1, 100),           true,  true,  Recs,  false, true);
    EXPECT(in(R, false, true, 0, 10, kQ, 100),               false, true,  Recs,  true,  true);   // nb == 2^28: compacted first
    EXPECT(in(R, false, true, 0, 10, 4, 100, 1),             false, true,  Recs,  true,  true);   // limitN 1
    EXPECT(in(R, false, true, 0, 10, 4, 100, 0, false),      false, true,  Recs,  true,  true);   // two parts
    // Records with cap == 0 (a buffer that is not page-locked): sorted straight
    // into outRecs, nothing copied during the pass, fetched afterwards
    EXPECT(in(R, false, true, 0, 10, 4, 0),                  true,  true,  None,  false, false);
    EXPECT(in(R, false, false, 10, 10, 4, 0),                true,  true,  None,  false, false);
    EXPECT(in(R, false, true, 0, 0, 4, 0),                   false, true,  None,  false, true);
}

// ---- one batch, the whole grid ----------------------------------------------

// What pass.cpp did before, from the flags of Ctx::Sink: `finish` chose the
// sort, `sinkBatch` chose the copy again from most of the same conditions.
struct OldFlags {
    bool sink, pinned, compact, recs, blockRecs;
};
static OldFlags oldFlags(const BatchIn& i) {
    switch (i.route) {
    case HitRoute::Device: return {false, false, false, false, false};
    case HitRoute::PinnedWhole: return {true, true, false, false, false};
    case HitRoute::Expander: return {true, i.wholeFallback, true, false, false};
    case HitRoute::Records: return {false, false, false, true, i.cap > 0};
    }
    std::abort();
}
struct OldPlan {
    bool direct, growRecs;
    BatchCopy copy;
    bool compactFirst, ok;
};
static OldPlan oldDecision(const BatchIn& i) {
    const OldFlags f = oldFlags(i);
    OldPlan o{};
    // finish
    const uint64_t end = i.nout + i.rows;
    const bool toExpander = !f.blockRecs && i.ok && end <= i.cap && f.compact && i.rows * 8 <= i.downSlot;
    const bool direct = (f.recs || toExpander) && i.limitN == 0 && i.onePart && i.nb < (1ull << 28);
    o.growRecs = direct || f.recs;
    o.direct = direct && i.rows;  // (batchDirect)
    // sinkBatch
    o.copy = BatchCopy::None;
    o.ok = i.ok;
    if (!i.ok || i.nout + i.rows > i.cap) {
        o.ok = false;
        return o;
    }
    const bool compact = f.compact && i.rows * 8 <= i.downSlot && i.nb < (1ull << 28);
    if (i.rows && f.blockRecs) o.copy = BatchCopy::RecordsDma, o.compactFirst = !direct;
    else if (i.rows && compact) o.copy = BatchCopy::ExpanderSlot, o.compactFirst = !direct;
    else if (i.rows && f.pinned) o.copy = BatchCopy::WholeDma;
    else if (i.rows) o.ok = false;
    return o;
}

static void checkGrid() {
    const uint64_t slot = 64;  // 8 records: the boundary within reach of small numbers
    uint64_t cases = 0;
    for (HitRoute route : {HitRoute::Device, HitRoute::PinnedWhole, HitRoute::Expander, HitRoute::Records})
        for (bool wholeFallback : {false, true})
            for (bool ok : {false, true})
                for (uint64_t nout : {0ull, 5ull})
                    for (uint64_t rows : {0ull, 1ull, 7ull, 8ull, 9ull})
                        for (uint64_t nb : {uint64_t(1), kQ - 1, kQ})
                            for (uint32_t limitN : {0u, 1u})
                                for (bool onePart : {true, false})
                                    for (int dc : {-1, 0, 1, 100}) {  // cap: end - 1, end, end + 1; 0
                                        const uint64_t end = nout + rows;
                                        if (dc < 0 && end == 0) continue;
                                        const uint64_t cap = dc == 100 ? 0 : end + dc;
                                        // (the old flags had no state for these two)
                                        if (route != HitRoute::Expander && wholeFallback) continue;
                                        if (route == HitRoute::Device && ok) continue;
                                        const BatchIn i{route, wholeFallback, ok, nout, rows, nb, cap, limitN, onePart, slot};
                                        const BatchPlan d = decideBatch(i);
                                        const OldPlan o = oldDecision(i);
                                        ++cases;
                                        // the same as before, for every input
                                        CHECK(d.direct == o.direct);
                                        CHECK(d.copy == o.copy);
                                        CHECK(d.ok == o.ok);
                                        CHECK(d.compactFirst == o.compactFirst);
                                        if (rows) CHECK(d.needRecs == o.growRecs);
                                        // what held only by reading finish and sinkBatch side by side:
                                        // a direct batch has nothing in `out`, so no whole DMA may take it
                                        if (d.direct) CHECK(d.copy != BatchCopy::WholeDma);
                                        // records leave from outRecs, or are compacted from `out` first
                                        if (d.copy == BatchCopy::RecordsDma || d.copy == BatchCopy::ExpanderSlot)
                                            CHECK(d.direct != d.compactFirst);
                                        else
                                            CHECK(!d.compactFirst);
                                        if (d.copy == BatchCopy::RecordsDma) CHECK(d.needRecs);  // copied out of outRecs
                                        if (d.direct) CHECK(d.needRecs && rows && limitN == 0 && onePart && nb < kQ);
                                        // a copy is issued only for rows that fit a sink that is in step
                                        if (d.copy != BatchCopy::None) CHECK(ok && d.ok && rows && end <= cap);
                                        if (!ok) CHECK(!d.ok);
                                        if (route == HitRoute::Device) CHECK(!d.direct && !d.needRecs && !d.ok);
                                        // --max_hits: the sort's side of the decision does not depend on
                                        // the rows, so deciding again with the rows kept cannot contradict it
                                        if (limitN) {
                                            BatchIn fewer = i;
                                            fewer.rows = rows / 2;
                                            const BatchPlan e = decideBatch(fewer);
                                            CHECK(!d.direct && !e.direct && e.needRecs == d.needRecs);
                                        }
                                    }
    if (cases < 2000) {
        std::fprintf(stderr, "grid too small: %llu cases\n", (unsigned long long)cases);
        ++failures;
    }
}

int main() {
    checkCallRoute();
    checkBatchByHand();
    checkGrid();
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
