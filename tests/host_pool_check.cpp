// The context's host pools alone (no HIP), for the thread and address
// sanitizers (test_host_pool.py): host_pool_check [rounds]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../sahara_amd/csrc/host_pool.h"

using namespace sahara;

static int fail(const char* what, long r) {
    std::fprintf(stderr, "%s: round %ld\n", what, r);
    return 1;
}

// One run of the pass's issuer / finisher handshake (issueAndFinish) over n
// batches: finish returns false at batch stopAt, issue / finish throw at
// batch issueThrow / finishThrow (-1: never). Every event gets a ticket from
// one clock; the handshake's own mutex orders the two threads' plain writes
// (a missing happens-before is what the thread sanitizer reports).
struct Thrown {
    char side;
    long batch;
};
static const char* handshake(long n, long window, long stopAt, long issueThrow, long finishThrow) {
    std::atomic<long> clock{1};
    std::vector<long> issueBegin(n, 0), issueEnd(n, 0), finBegin(n, 0), finEnd(n, 0);
    long setups = 0, trails = 0, joins = 0, finished = 0, issuedN = 0;
    const char *issueBad = nullptr, *finBad = nullptr;  // what each thread saw go wrong
    char caught = 0;
    long caughtAt = -1;
    try {
        issueAndFinish(
            (uint64_t)n, (uint64_t)window, [&] { ++setups; },
            [&](uint64_t b) {
                issueBegin[b] = clock++;
                if ((long)b >= window && !finEnd[b - window]) issueBad = "issue(b) started before finish(b - window) returned";
                if ((long)b != issuedN) issueBad = "issue out of order";
                if ((long)b == issueThrow) throw Thrown{'i', (long)b};
                ++issuedN;
                issueEnd[b] = clock++;
            },
            [&](uint64_t f) {
                finBegin[f] = clock++;
                if ((long)f != finished) finBad = "finish out of order";
                if (!issueEnd[f]) finBad = "finish(f) before issue(f) returned";
                if ((long)f == finishThrow) throw Thrown{'f', (long)f};
                ++finished;
                finEnd[f] = clock++;
                return (long)f != stopAt;
            },
            [&] { ++trails; }, [&] { ++joins; });
    } catch (const Thrown& t) {
        caught = t.side;
        caughtAt = t.batch;
    }
    if (issueBad || finBad) return issueBad ? issueBad : finBad;
    if (setups != 1 || joins != 1) return "setup and the after-join step run once each";
    for (long b = 0; b < n; ++b) {
        if (finBegin[b] && finBegin[b] < issueEnd[b]) return "finish(f) began before issue(f) returned";
        if (b >= window && issueBegin[b] && issueBegin[b] < finEnd[b - window]) return "issue ran past the window";
    }
    const bool finThrew = finishThrow >= 0 && finishThrow < n && finBegin[finishThrow];
    const bool issueThrew = issueThrow >= 0 && issueThrow < n && issueBegin[issueThrow];
    if (issueThrew ? (caught != 'i' || caughtAt != issueThrow) : finThrew ? (caught != 'f' || caughtAt != finishThrow) : caught != 0)
        return "the caller sees the issuer's exception, else the finisher's, else none";
    if (trails != (finThrew ? 0 : 1)) return "the trailing step runs once unless finish threw";
    if (!issueThrew && !finThrew) {
        const long want = stopAt >= 0 && stopAt < n ? stopAt + 1 : n;
        if (finished != want) return "finish sees 0 .. n-1 in order, none after the one that returned false";
        if (issuedN < want || issuedN > std::min(n, want + window))
            return "at most `window` batches are issued after the one whose finish returned false";
    }
    return nullptr;
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? std::atol(argv[1]) : 20000;
    for (long r = 0; r < rounds / 4; ++r) {  // the handshake: n in 0..13, window in 1..5
        const long n = r % 14, window = 1 + (r / 14) % 5, mode = (r / 70) % 5, at = n ? (r / 350) % n : 0;
        // plain; finish returns false at `at`; issue throws; finish throws; both throw
        const char* bad = handshake(n, window, mode == 1 ? at : -1, mode == 2 || mode == 4 ? at : -1,
                                    mode == 3 ? at : mode == 4 ? std::max(0L, at - 1) : -1);
        if (bad) {
            std::fprintf(stderr, "n %ld window %ld mode %ld at %ld: ", n, window, mode, at);
            return fail(bad, r);
        }
    }
    {  // fork-join over a group on the stack, as staging.cpp runPieces does
        TaskPool P(8);
        std::vector<long> slot(13);
        for (long r = 0; r < rounds; ++r) {
            const size_t n = 1 + (size_t)(r % 13);
            TaskGroup g;
            g.begin(n);
            std::vector<std::function<void()>> fs;
            for (size_t k = 0; k < n; ++k)
                fs.emplace_back([&slot, &g, k, r] {
                    slot[k] = r + (long)k;
                    g.oneDone();
                });
            P.postMany(fs);
            g.wait();
            for (size_t k = 0; k < n; ++k)
                if (slot[k] != r + (long)k) return fail("TaskGroup", r);
        }
    }
    {  // HostPool::run: 7 workers and the caller
        HostPool H(7);
        std::vector<long> slot(H.size());
        for (long r = 0; r < rounds; ++r) {
            H.run([&](unsigned t) { slot[t] = r + t; });
            for (unsigned t = 0; t < H.size(); ++t)
                if (slot[t] != r + t) return fail("HostPool", r);
        }
    }
    {  // a pool destroyed with tasks still queued drops them and ends
        std::vector<long> slot(1000);
        TaskPool P(2);
        for (size_t k = 0; k < slot.size(); ++k) P.post([&slot, k] { slot[k] = 1; });
    }
    std::puts("OK");
    return 0;
}
