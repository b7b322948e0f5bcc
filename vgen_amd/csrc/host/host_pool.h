// host_pool.h — threads for the host-side work of a scan (scanner.cpp): how many, and the pool that confirms candidates.
#pragma once
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace vg {

// Threads for host-side work (candidate confirmation, rendering): the cores this process may really use — affinity mask,
// capped by a cgroup-v2 CPU quota —, not the machine's thread count (a 256-thread host with a 16-core quota ran 256 workers).
inline unsigned host_threads() {
    unsigned n = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n ? n : 1024, (unsigned)CPU_COUNT(&set));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32];
        long period = 0;
        if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
            n = std::min<unsigned>(n, (unsigned)std::max(1L, atol(quota) / period));
        fclose(f);
    }
    return std::max(1u, std::min(n, 64u));
}

// Host-side filtering of full dumps (the reference's rayon par_iter over every hash of a batch,
// src/gpu.rs:1030-1093): a pool of worker threads that lives as long as the scan, handed one index range per
// thread and batch.
class HostFilterPool {
public:
    explicit HostFilterPool(unsigned n) : n_(std::max(1u, n)) {
        for (unsigned t = 0; t < n_; t++) th_.emplace_back([this, t]() { loop(t); });
    }
    ~HostFilterPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
            gen_++;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    unsigned size() const { return n_; }
    // runs fn(t) on every worker t and returns when all are done
    void run(const std::function<void(unsigned)> &fn) {
        std::unique_lock<std::mutex> g(mu_);
        fn_ = &fn;
        pending_ = n_;
        gen_++;
        cv_.notify_all();
        done_.wait(g, [this]() { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void loop(unsigned t) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(unsigned)> *fn;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&]() { return gen_ != seen; });
                seen = gen_;
                if (quit_) return;
                fn = fn_;
            }
            (*fn)(t);
            {
                std::lock_guard<std::mutex> g(mu_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    unsigned n_;
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned)> *fn_ = nullptr;
    unsigned pending_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};

}  // namespace vg
