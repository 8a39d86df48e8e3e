// taskpool.h -- the host worker threads of the set-up code and the two range helpers built on them.  Includes nothing from
// HIP: host.h includes it for the library, aggregation.cpp and tests/cxx/test_aggregation.cpp (which also runs under the
// thread and address sanitizers) include it directly.
#pragma once
#include "options.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <pthread.h>
#include <sched.h>
#include <thread>
#include <vector>

namespace dpgo_host {

// Host worker threads of the set-up code (the hierarchy's symbolic set-up): created once per process and kept -- in a
// process that has the HIP runtime and an ML framework loaded pthread_create costs 0.2-0.4 ms (static TLS of every loaded
// library), more than the sections it would run.  A batch = fn(0 .. count-1); whoever waits for a batch executes its items
// too, so batches may be started from inside items (nested sections) without a deadlock.
class TaskPool {
 public:
  struct Batch {
    std::function<void(int)> fn;
    int count = 0;
    std::atomic<int> next{0}, done{0};
  };
  using Job = std::shared_ptr<Batch>;
  static TaskPool& get() {
    static TaskPool* pool = new TaskPool();  // never destroyed: the workers are detached
    return *pool;
  }
  // starts fn(0 .. count-1) on the workers; the caller goes on and later calls wait()
  Job submit(int count, std::function<void(int)> fn, int max_threads) {
    Job b = std::make_shared<Batch>();
    b->fn = std::move(fn);
    b->count = count;
    const int helpers = std::max(0, std::min(count, max_threads - 1));
    if (helpers > 0) {
      {
        std::lock_guard<std::mutex> lk(mu_);
        while ((int)nworkers_ < std::min(kMaxWorkers, std::max(helpers, (int)nworkers_))) {
          const int id = (int)nworkers_;
          std::thread([this, id] {
            pin(id);
            loop();
          }).detach();
          ++nworkers_;
        }
        for (int k = 0; k < helpers; ++k) queue_.push_back(b);
      }
      cv_.notify_all();
    }
    return b;
  }
  // executes what is left of the batch, then waits for the items other threads are still running
  void wait(const Job& b) {
    if (!b) return;
    help(*b);
    while (b->done.load(std::memory_order_acquire) < b->count) std::this_thread::yield();
  }
  void run(int count, const std::function<void(int)>& fn, int max_threads) {
    if (count <= 0) return;
    if (count == 1 || max_threads <= 1) {
      for (int k = 0; k < count; ++k) fn(k);
      return;
    }
    wait(submit(count, fn, max_threads));
  }
  // creates the workers ahead of their first use, from a helper thread (the caller pays one pthread_create)
  void warm(int threads) {
    bool expected = false;
    if (threads <= 1 || !warmed_.compare_exchange_strong(expected, true)) return;
    std::thread([this, threads] { wait(submit(threads - 1, [](int) {}, threads)); }).detach();
  }

 private:
  static constexpr int kMaxWorkers = 15;
  // Workers next to the thread that created the pool (DPGO_SETUP_PIN=0: wherever the scheduler puts them): the sections
  // they run share arrays of a few MB that thread has just written -- on a multi-socket host a worker on another socket
  // (or another L3 slice) reads them across the fabric.  Heuristic: the aligned group of 8 consecutive CPU numbers around
  // the creator's CPU (one core complex on current server parts), restricted to the process's affinity mask; a worker may
  // run on any CPU of the group.  Purely a placement hint: failures are ignored.
  int home_cpu_ = -1;
  void pin(int) {
    if (!pin_enabled() || home_cpu_ < 0) return;
    cpu_set_t allowed, want;
    CPU_ZERO(&allowed);
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
    const int lo = home_cpu_ & ~7;
    int cnt = 0;
    for (int c = lo; c < lo + 8; ++c)
      if (c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) CPU_SET(c, &want), ++cnt;
    if (cnt >= 2) (void)pthread_setaffinity_np(pthread_self(), sizeof(want), &want);
  }
  static bool pin_enabled() { return options().setup_pin != 0; }
  TaskPool() { home_cpu_ = sched_getcpu(); }
  static void help(Batch& b) {
    for (;;) {
      const int k = b.next.fetch_add(1, std::memory_order_relaxed);
      if (k >= b.count) return;
      b.fn(k);
      b.done.fetch_add(1, std::memory_order_release);
    }
  }
  void loop() {
    for (;;) {
      Job b;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !queue_.empty(); });
        b = std::move(queue_.front());
        queue_.erase(queue_.begin());
      }
      help(*b);
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Job> queue_;
  unsigned nworkers_ = 0;
  std::atomic<bool> warmed_{false};
};
// waits for a job when the scope is left, whichever way
struct JobGuard {
  TaskPool::Job job;
  ~JobGuard() { TaskPool::get().wait(job); }
};

// Host threads of the symbolic set-up (DPGO_SETUP_THREADS; the results do not depend on the count: every parallel section
// works on disjoint row ranges and is joined in range order).
inline int setup_threads() {
  const int want = options().setup_threads;
  if (want > 0) return std::min(want, 64);
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(8u, hw ? hw : 1u));
}
// fn(chunk, begin, end) over `chunks` contiguous ranges of [0, n) on the process's worker threads (TaskPool)
template <class F>
void parallel_ranges(int n, int chunks, F&& fn) {
  chunks = std::max(1, std::min(chunks, n > 0 ? n : 1));
  TaskPool::get().run(chunks, [&](int c) {
    fn(c, (int)((long long)n * c / chunks), (int)((long long)n * (c + 1) / chunks));
  }, setup_threads());
}
// rows [lo, hi) of a row-wise pattern built by `row(chunk, i, out)` (appends row i's sorted columns) into per-range pieces,
// joined in range order: rowptr / colidx identical to the serial loop
template <class F>
void pattern_by_ranges(int n, int threads, int grain, size_t reserve_hint, F&& row, std::vector<int32_t>& rowptr_out,
                       std::vector<int32_t>& col_out) {
  const int chunks = std::max(1, std::min(threads, n / grain + 1));
  std::vector<std::vector<int32_t>> cols(chunks), cnt(chunks);
  parallel_ranges(n, chunks, [&](int c, int lo, int hi) {
    auto& cc = cols[c];
    auto& nn = cnt[c];
    cc.reserve(reserve_hint / chunks + 16);
    nn.resize(hi - lo);
    for (int i = lo; i < hi; ++i) {
      const size_t first = cc.size();
      row(c, i, cc);
      nn[i - lo] = (int32_t)(cc.size() - first);
    }
  });
  rowptr_out.assign(n + 1, 0);
  size_t total = 0;
  for (auto& cc : cols) total += cc.size();
  col_out.resize(total);
  std::vector<size_t> base(chunks + 1, 0);
  for (int c = 0; c < chunks; ++c) base[c + 1] = base[c] + cols[c].size();
  parallel_ranges(chunks, chunks, [&](int, int c0, int c1) {
    for (int c = c0; c < c1; ++c) {
      const int lo = (int)((long long)n * c / chunks);
      if (!cols[c].empty()) std::memcpy(col_out.data() + base[c], cols[c].data(), sizeof(int32_t) * cols[c].size());
      size_t at = base[c];
      for (size_t k = 0; k < cnt[c].size(); ++k) {
        at += cnt[c][k];
        rowptr_out[lo + k + 1] = (int32_t)at;
      }
    }
  });
}

}  // namespace dpgo_host
