// host_pool.h — the host thread pools of a context and where their threads
// run. No HIP here: tests/host_pool_check.cpp builds this header alone under
// the thread and address sanitizers.
#pragma once
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace sahara {

// NUMA placement of a context's own host threads that touch its pinned
// buffers (the pass's finisher, the hit expander, the ring pinning): the CPUs
// of the NUMA node the GPU hangs off (/sys/bus/pci/devices/<bdf>/numa_node),
// as far as the process may use them. The packing pool reads the caller's
// buffers, wherever those are, and stays unbound (staging.cpp hostPool).
// node = -1 (unknown, or SAHARA_NUMA=0): threads stay where the OS puts them.
struct Placement {
    int node = -1;
    int ncpus = 0;      // CPUs the context's threads are bound to (0: not bound)
    cpu_set_t cpus;
    Placement() { CPU_ZERO(&cpus); }
    void bind() const {
        if (ncpus > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpus), &cpus);
    }
};

// Host worker threads of a context (pattern packing for the upload), started
// once: a streamed upload packs several chunks per call, and fresh threads per
// chunk measured slower than the link.
class HostPool {
public:
    explicit HostPool(unsigned workers, const Placement* pl = nullptr) {
        for (unsigned i = 1; i <= workers; ++i)
            ts_.emplace_back([this, i, pl] {
                if (pl) pl->bind();
                loop(i);
            });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : ts_) t.join();
    }
    unsigned size() const { return (unsigned)ts_.size() + 1; }
    // f(t) for every t in [0, size()), t = 0 on the calling thread; f must not throw
    void run(const std::function<void(unsigned)>& f) {
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = &f;
            pending_ = (unsigned)ts_.size();
            ++gen_;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
    }

private:
    void loop(unsigned id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(unsigned)>* f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                f = job_;
            }
            (*f)(id);
            std::lock_guard<std::mutex> g(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> ts_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned)>* job_ = nullptr;
    uint64_t gen_ = 0;
    unsigned pending_ = 0;
    bool stop_ = false;
};

// Host threads that pack the streamed upload (staging.cpp): a FIFO of tasks
// rather than fork-join rounds, so that the pieces of several chunks are in
// flight at once. A fork-join round per chunk (13 pieces of 4M symbols on 16
// threads at C3) left threads idle at every chunk's end and stopped packing
// whenever the issuing thread was not inside it; queued chunks keep every
// thread busy while the issuing thread enqueues kernels or waits for a slot.
class TaskPool {
public:
    explicit TaskPool(unsigned workers, const Placement* pl = nullptr) {
        for (unsigned i = 0; i < std::max(workers, 1u); ++i)
            ts_.emplace_back([this, pl] {
                if (pl) pl->bind();
                loop();
            });
    }
    ~TaskPool() {  // tasks still queued are dropped (callers wait for theirs first)
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : ts_) t.join();
    }
    unsigned size() const { return (unsigned)ts_.size(); }
    void post(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }
    void postMany(std::vector<std::function<void()>>& fs) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (auto& f : fs) q_.push_back(std::move(f));
        }
        cv_.notify_all();
        fs.clear();
    }

private:
    void loop() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (stop_) return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::vector<std::thread> ts_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool stop_ = false;
};

// A group of tasks posted to a TaskPool that the poster waits for. The count
// lives under the mutex, and the last task notifies while it still holds it:
// once wait() has returned no task touches the group again, so it may sit on
// the waiter's stack (staging.cpp runPieces). A lock-free count let wait()
// return, and the group die, while the last task was still on its way to
// lock the mutex.
struct TaskGroup {
    uint64_t left = 0;
    std::mutex mu;
    std::condition_variable cv;
    void begin(uint64_t n) {
        std::lock_guard<std::mutex> g(mu);
        left = n;
    }
    void oneDone() {
        std::lock_guard<std::mutex> g(mu);
        if (--left == 0) cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return left == 0; });
    }
};

// The issuer / finisher handshake of a pipelined pass (pass.cpp runPass). The
// calling thread runs issue(b) for b = 0 .. n-1, never more than `window`
// batches ahead of the last finished one; a second thread runs setup(), then
// finish(f) in order, each after issue(f) has returned, then trail() once. A
// finish that returns false stops both sides (the pass overflowed). An
// exception on either side stops the other and is rethrown here after the
// join, the issuer's if both threw. afterJoin() runs on the calling thread
// between the join and the rethrow (the pass waits for its streams there).
template <class Setup, class Issue, class Finish, class Trail, class AfterJoin>
void issueAndFinish(uint64_t n, uint64_t window, Setup&& setup, Issue&& issue, Finish&& finish, Trail&& trail,
                    AfterJoin&& afterJoin) {
    std::mutex mu;
    std::condition_variable cv;
    uint64_t issued = 0, released = 0;  // batches issued; batches finished
    bool stop = false;
    std::exception_ptr finErr, issueErr;
    std::thread finisher([&] {
        try {
            setup();
            for (uint64_t f = 0; f < n; ++f) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return issued > f || stop; });
                    if (issued <= f) break;
                }
                const bool go = finish(f);
                {
                    std::lock_guard<std::mutex> g(mu);
                    released = f + 1;
                    if (!go) stop = true;
                }
                cv.notify_all();
                if (!go) break;
            }
            trail();
        } catch (...) {
            finErr = std::current_exception();
        }
        std::lock_guard<std::mutex> g(mu);
        stop = true;
        cv.notify_all();
    });
    try {
        for (uint64_t b = 0; b < n; ++b) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return b < released + window || stop; });
                if (stop) break;
            }
            issue(b);
            {
                std::lock_guard<std::mutex> g(mu);
                issued = b + 1;
            }
            cv.notify_all();
        }
    } catch (...) {
        issueErr = std::current_exception();
    }
    {
        std::lock_guard<std::mutex> g(mu);
        if (issueErr) stop = true;
    }
    cv.notify_all();
    finisher.join();
    afterJoin();
    if (issueErr) std::rethrow_exception(issueErr);
    if (finErr) std::rethrow_exception(finErr);
}

}  // namespace sahara
