// The context's host pools alone (no HIP), for the thread and address
// sanitizers (test_host_pool.py): host_pool_check [rounds]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../sahara_amd/csrc/host_pool.h"

using namespace sahara;

static int fail(const char* what, long r) {
    std::fprintf(stderr, "%s: round %ld\n", what, r);
    return 1;
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? std::atol(argv[1]) : 20000;
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
