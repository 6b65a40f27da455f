// hit_route.h — where a call's hits go while its pass runs, as a value, and
// the two pure functions that decide it: the route of a call (callRoute) and
// what one batch does on that route (decideBatch). No HIP, like pass_plan.h:
// tests/hit_route_check.cpp builds this header alone. Nothing else in the
// library derives a destination from the call's state.
#pragma once
#include <cstdint>

namespace sahara {

enum class HitRoute {
    Device,       // no host sink during the pass: hits stay on the device (sahara_gpu_run, the host besthits
                  // loop, every pass of a multi-part index, the host-limited --max_hits, no sink to be had)
    PinnedWhole,  // whole hits, each batch by DMA into a pinned host buffer
    Expander,     // 8-B records through the download ring, expanded into the host buffer by the Expander
    Records,      // 8-B records by DMA into the compact call's pinned block buffer
};

// Whether a pass starts with its sink in step ("every batch so far went into
// the sink"). A Records sink that is not page-locked has cap 0: it falls out
// of step at the first batch with a hit.
inline bool sinkStarts(HitRoute r) { return r != HitRoute::Device; }

// The route of a whole-hit call (sahara_gpu_search and its kin) from the
// buffer it got. Hits go whole into a pinned sink (DMA; no host CPU or memory
// traffic beyond the write), or, into pageable memory, as 8-B records that
// host threads expand: a third of the PCIe bytes, but the expansion reads and
// writes host memory the packing also needs (at C3 it took ~4 ms per batch
// beside the packing, 300M against 330M reads/s). forceFull / forceCompact:
// SAHARA_FULL_DOWNLOAD=1 / SAHARA_COMPACT_DOWNLOAD=1.
struct CallRoute {
    HitRoute route;
    bool wholeFallback;  // Expander into a pinned sink: a batch that fits no ring slot goes by whole DMA
};
inline CallRoute callRoute(bool pinned, bool compactOk, bool forceFull, bool forceCompact) {
    if (compactOk && !forceFull && (!pinned || forceCompact)) return {HitRoute::Expander, pinned};
    return {pinned ? HitRoute::PinnedWhole : HitRoute::Device, false};
}

// The one copy a batch issues on stream stF.
enum class BatchCopy { None, RecordsDma, ExpanderSlot, WholeDma };

struct BatchIn {
    HitRoute route;
    bool wholeFallback;    // CallRoute's
    bool ok;               // every batch so far went into the sink
    uint64_t nout, rows;   // the call's hits before this batch; this batch's
    uint64_t nb;           // this batch's patterns
    uint64_t cap;          // hits (records) the sink holds
    uint32_t limitN;       // --max_hits per batch on the device, 0: off
    bool onePart;          // a single-part index
    uint64_t downSlot;     // bytes of a download ring slot (Ctx::kDownSlot)
    bool loci = false;     // the loci stage runs on the batch's whole hits (loci.hip)
    bool pairs = false;    // the pair stage runs on them (pairs.hip)
};

struct BatchPlan {
    bool direct;        // sorted straight into compact records (outRecs): `out` gets nothing of the batch
    bool needRecs;      // outRecs must hold the batch (at its place among the call's hits)
    BatchCopy copy;
    bool compactFirst;  // the copy's records are made from the whole hits first (kCompactHits): not direct
    bool ok;            // the sink's new state
};

// A compact record holds the batch-local query in 28 bits and the sort can
// write it only where nothing reads the whole hit on the device afterwards:
// no loci stage, no pair stage, no --max_hits cut, no merge of parts. loci,
// pairs and limitN != 0 each make direct and needRecs independent of rows, so
// a batch decided again with the rows those stages kept (Pass::finish) cannot
// contradict its sort.
inline BatchPlan decideBatch(const BatchIn& in) {
    constexpr uint64_t kRecQueries = 1ull << 28;
    const bool fits = in.ok && in.route != HitRoute::Device && in.nout + in.rows <= in.cap;
    const bool slotFits = in.rows * sizeof(uint64_t) <= in.downSlot;
    const bool takesRecs = in.route == HitRoute::Records || (in.route == HitRoute::Expander && fits && slotFits);
    BatchPlan d{};
    d.direct = in.rows && takesRecs && !in.loci && !in.pairs && in.limitN == 0 && in.onePart && in.nb < kRecQueries;
    d.needRecs = d.direct || in.route == HitRoute::Records;
    d.copy = BatchCopy::None;
    d.ok = fits;
    if (fits && in.rows) {
        if (in.route == HitRoute::Records) d.copy = BatchCopy::RecordsDma;
        else if (in.route == HitRoute::Expander && slotFits && in.nb < kRecQueries) d.copy = BatchCopy::ExpanderSlot;
        else if (in.route == HitRoute::PinnedWhole || in.wholeFallback) d.copy = BatchCopy::WholeDma;
        else d.ok = false;  // neither fits: the rest goes after the pass
    }
    d.compactFirst = (d.copy == BatchCopy::RecordsDma || d.copy == BatchCopy::ExpanderSlot) && !d.direct;
    return d;
}

}  // namespace sahara
