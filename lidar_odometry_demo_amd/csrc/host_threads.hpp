// Host threads of the odometry: the worker pool of the per-point host stages, the helper thread of the deferred
// keyframe update, and the stage timer of LOM_DEBUG_TIMING.  Standard library only.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <ctime>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/lidar_odometry_amd.h"

namespace lom {

// LOM_DEBUG_TIMING=1 (read once, by lom_odometry_create): per-stage wall times of processCloud on stderr
struct StageTimer {
    bool on;
    double t0 = now(), last = t0;
    explicit StageTimer(bool enabled) : on(enabled) {}
    static double now()
    {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    }
    void lap(const char *what)
    {
        if (!on) return;
        const double t = now();
        std::fprintf(stderr, "  %-14s %8.1f us\n", what, (t - last) * 1e6);
        last = t;
    }
    void total()
    {
        if (on) std::fprintf(stderr, "processCloud total %8.1f us\n", (now() - t0) * 1e6);
    }
};

// ---- host worker pool -------------------------------------------------------------
// The reference runs its per-point transforms under std::execution::par
// (point_time_normalize.h:31, cloud_transform.h:21); this is the same idea without TBB.
// Work is split into contiguous index ranges, so results do not depend on the thread count.
class Pool {
public:
    explicit Pool(unsigned n_threads)
    {
        for (unsigned i = 1; i < n_threads; i++) start(i);
    }
    ~Pool()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
            generation_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    unsigned size() const { return (unsigned)workers_.size() + 1; }

    // fn(begin, end, part) over [0, n) in size() contiguous parts; the caller takes part 0,
    // worker w always takes part w.  Workers spin for a while after each job (a frame issues
    // five of these within a millisecond) and park on a condition variable when idle longer.
    template <typename F>
    void parallel_for(size_t n, F &&fn, size_t serial_below = 2048)
    {
        const unsigned parts = size();
        if (parts == 1 || n < serial_below) {
            fn(size_t(0), n, 0u);
            return;
        }
        std::function<void(unsigned)> job = [&](unsigned p) { fn(n * p / parts, n * (p + 1) / parts, p); };
        job_ = &job;
        pending_.store(parts - 1, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> l(m_);  // pairs with the parked workers' predicate check
            generation_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        job(0);
        while (pending_.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
        job_ = nullptr;
    }

private:
    // host_threads.cpp; out of line and hidden, so that std::thread's instantiation for it is no exported symbol
    __attribute__((visibility("hidden"))) void start(unsigned part);
    void run(unsigned part)
    {
        unsigned long seen = 0;
        for (;;) {
            // spin ~100 us for the next job, then park
            unsigned long g = seen;
            for (int spin = 0; spin < 40000 && (g = generation_.load(std::memory_order_acquire)) == seen; spin++)
                __builtin_ia32_pause();
            if (g == seen) {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return generation_.load(std::memory_order_acquire) != seen; });
                g = generation_.load(std::memory_order_acquire);
            }
            seen = g;
            if (stop_) return;
            (*job_)(part);
            pending_.fetch_sub(1, std::memory_order_release);
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_;
    const std::function<void(unsigned)> *job_ = nullptr;
    std::atomic<unsigned> pending_{0};
    std::atomic<unsigned long> generation_{0};
    bool stop_ = false;
};

template <typename F>
void run_parts(Pool *pool, size_t n, F &&fn, size_t serial_below = 2048)
{
    if (pool)
        pool->parallel_for(n, fn, serial_below);
    else
        fn(size_t(0), n, 0u);
}

}  // namespace lom

// (At global scope, as it always was: the exported symbols of std::thread's instantiation for it carry its name.)
// One helper thread per odometry: the keyframe update of frame k (radiusCleanup, rigid transform,
// insert: lidar_odometry.cpp:67-70) does not influence frame k's pose, and frame k+1 touches the
// GPU handles only after its host stages (time normalisation, deskew, classifier, range filter).
// So processCloud returns the pose and lets the update run here; the next call (or any accessor)
// joins it before it uses a handle.  Same operations in the same order on the same stream: results
// do not change.
class Deferred {
public:
    Deferred() : th_([this] { loop(); }) {}
    ~Deferred()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void submit(std::function<int()> f)
    {
        bool asleep;
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = std::move(f);
            busy_ = true;
            asleep = asleep_;
        }
        running_.store(true, std::memory_order_release);
        posted_.store(true, std::memory_order_release);
        if (asleep) cv_.notify_all();
    }
    int join()  // status of the last job (LOM_OK if none is pending)
    {
        // a job is a few tens of microseconds of enqueues and two looks at the device: watch for its end
        // before going to sleep on it (a futex wake-up costs as much as the job)
        for (int i = 0; i < kSpins && running_.load(std::memory_order_acquire); i++) __builtin_ia32_pause();
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !busy_; });
        const int rc = rc_;
        rc_ = LOM_OK;
        return rc;
    }

private:
    void loop()
    {
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            // frames that follow each other closely find the worker awake: it watches for the next job for
            // about half a millisecond before it sleeps on the condition variable (10 Hz input: asleep 99 %)
            g.unlock();
            for (int i = 0; i < kSpins && !posted_.load(std::memory_order_acquire); i++) __builtin_ia32_pause();
            g.lock();
            asleep_ = true;
            cv_.wait(g, [this] { return stop_ || (busy_ && job_); });
            asleep_ = false;
            if (stop_) return;
            posted_.store(false, std::memory_order_relaxed);
            std::function<int()> f = std::move(job_);
            job_ = nullptr;
            g.unlock();
            const int rc = f();
            g.lock();
            rc_ = rc;
            busy_ = false;
            running_.store(false, std::memory_order_release);
            cv_.notify_all();
        }
    }
    static constexpr int kSpins = 20000;  // x one `pause` (about 25 ns)
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    std::atomic<bool> posted_{false}, running_{false};  // a job waits for the worker / is not finished yet
    bool busy_ = false, stop_ = false, asleep_ = false;
    int rc_ = LOM_OK;
    std::thread th_;
};
