// A pool of host threads that run jobs ahead of an in-order consumer, each into one of a bounded
// set of slots (the worker's kind-4 preflights, r0hip_worker_set_preflight_threads). Host-only:
// plain C++17, no HIP. The job type, the slot type, the work function and the slot allocator are
// the user's, so a stand-alone program can drive the pool with malloc-backed slots.
//
//   producer   push(job)        in ticket order; never blocks
//   pool       a thread takes a free slot and the next queued job under one lock, so slots go to
//              jobs in ticket order; with no free slot it blocks. It runs work(job, slot, &msg):
//                kReady   the slot holds the job's result and stays with the job
//                kFailed  msg is the job's error; the slot is returned
//                kLeft    the job is left to the consumer (nothing was run); the slot is returned
//              (a throw from work counts as kFailed with the exception's message)
//   consumer   take(job)        the queue's front job, which must be `job`: blocks until a pool
//                               thread has finished it and removes it from the queue
//   releaser   release(slot)    once the result has been read; any thread
//
// Look-ahead is bounded by the slots: at most `slots` results exist at a time. No deadlock as long
// as the consumer takes jobs in push order and every kReady slot is released without waiting for
// a later job: the earliest job not yet taken either holds a slot or gets the next one returned.
// resize() and stop() are for an idle pool (everything pushed has been taken): the queue is empty,
// so the threads only wait and can be joined at once; slots still held by releasers are waited for.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace r0 {

enum class PoolVerdict : uint8_t { kReady, kFailed, kLeft };

struct PreflightPoolStats {
  uint32_t threads = 0, slots = 0, peak_slots_in_use = 0;
  uint64_t jobs = 0;    // jobs a pool thread ran (kReady or kFailed)
  uint64_t left = 0;    // jobs left to the consumer
  double busy_ms = 0;   // summed over the threads, inside work
};

template <typename Job, typename Slot>
class PreflightPool {
 public:
  using Work = std::function<PoolVerdict(Job*, Slot&, std::string*)>;
  using MakeSlot = std::function<Slot*()>;
  using FreeSlot = std::function<void(Slot*)>;
  struct Taken {
    PoolVerdict verdict = PoolVerdict::kLeft;
    long slot = -1;     // kReady: the index to read with slot() and to give back with release()
    std::string error;  // kFailed
  };

  PreflightPool(Work work, MakeSlot make_slot, FreeSlot free_slot)
      : work_(std::move(work)), make_slot_(std::move(make_slot)), free_slot_(std::move(free_slot)) {}
  PreflightPool(const PreflightPool&) = delete;
  PreflightPool& operator=(const PreflightPool&) = delete;
  ~PreflightPool() { stop(); }

  uint32_t threads() const {
    std::lock_guard<std::mutex> lk(mu_);
    return uint32_t(threads_.size());
  }
  bool idle() const {
    std::lock_guard<std::mutex> lk(mu_);
    return q_.empty();
  }

  // n threads and n + in_flight + 1 slots (n == 0: none of either). The pool must be idle. The
  // counters run on, except the peak of slots in use, which restarts with the new slots.
  void resize(uint32_t n, uint32_t in_flight) {
    stop();
    std::lock_guard<std::mutex> lk(mu_);
    stats_.peak_slots_in_use = 0;
    if (n == 0) return;
    const size_t count = size_t(n) + in_flight + 1;
    slots_.reserve(count);
    for (size_t i = 0; i < count; i++) {
      slots_.push_back(make_slot_());
      free_.push_back(long(i));
    }
    stopping_ = false;
    for (uint32_t t = 0; t < n; t++) threads_.emplace_back([this] { run(); });
  }

  // Joins the threads and frees the slots. Jobs still queued are run first (by the threads, as
  // long as a consumer keeps taking them); slots not yet released are waited for.
  void stop() {
    std::vector<std::thread> threads;
    {
      std::lock_guard<std::mutex> lk(mu_);
      stopping_ = true;
      threads.swap(threads_);
    }
    cv_work_.notify_all();
    for (auto& t : threads) t.join();
    std::unique_lock<std::mutex> lk(mu_);
    cv_slot_.wait(lk, [&] { return free_.size() == slots_.size(); });
    for (Slot* s : slots_) free_slot_(s);
    slots_.clear();
    free_.clear();
    in_use_ = 0;
  }

  // false: the pool has no threads and the job is the consumer's own
  bool push(Job* job) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (threads_.empty() || stopping_) return false;
      q_.emplace_back();
      q_.back().job = job;
    }
    cv_work_.notify_one();
    return true;
  }

  Taken take(Job* job) {
    std::unique_lock<std::mutex> lk(mu_);
    if (q_.empty() || q_.front().job != job) throw std::logic_error("preflight pool: jobs are taken in push order");
    cv_done_.wait(lk, [&] { return q_.front().state == kDone; });
    Taken t;
    t.verdict = q_.front().verdict;
    t.slot = q_.front().slot;
    t.error = std::move(q_.front().error);
    q_.pop_front();
    started_--;
    return t;
  }

  // the slot of a kReady job, until release(): only its holder reads or writes it
  Slot& slot(long i) { return *slots_[size_t(i)]; }

  void release(long i) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      free_.push_back(i);
      in_use_--;
    }
    cv_work_.notify_all();
    cv_slot_.notify_all();
  }

  // f(const Slot&) on every slot, free or held: it may read only what a holder writes atomically
  template <typename F>
  PreflightPoolStats stats(F f) const {
    std::lock_guard<std::mutex> lk(mu_);
    PreflightPoolStats s = stats_;
    s.threads = uint32_t(threads_.size());
    s.slots = uint32_t(slots_.size());
    for (const Slot* p : slots_) f(*p);
    return s;
  }

 private:
  enum State : uint8_t { kQueued, kRunning, kDone };
  struct Entry {
    Job* job = nullptr;
    State state = kQueued;
    PoolVerdict verdict = PoolVerdict::kLeft;
    long slot = -1;
    std::string error;
  };

  void run() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      // a free slot and the next job under one lock: slots go to jobs in push order
      cv_work_.wait(lk, [&] { return (started_ < q_.size() && !free_.empty()) || (stopping_ && started_ == q_.size()); });
      if (started_ == q_.size()) return;
      Entry& e = q_[started_++];  // a deque: the reference outlives pushes and pops of other entries
      const long s = free_.front();
      free_.pop_front();
      in_use_++;
      if (in_use_ > stats_.peak_slots_in_use) stats_.peak_slots_in_use = in_use_;
      e.state = kRunning;
      e.slot = s;
      Job* const job = e.job;
      Slot& slot = *slots_[size_t(s)];
      lk.unlock();
      std::string msg;
      PoolVerdict v;
      const auto t0 = std::chrono::steady_clock::now();
      try {
        v = work_(job, slot, &msg);
      } catch (const std::exception& ex) {
        v = PoolVerdict::kFailed, msg = ex.what();
      } catch (...) {
        v = PoolVerdict::kFailed, msg = "preflight pool: unknown error";
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      lk.lock();
      e.verdict = v;
      e.error = std::move(msg);
      if (v == PoolVerdict::kLeft) {
        stats_.left++;
      } else {
        stats_.jobs++;
        stats_.busy_ms += ms;
      }
      if (v != PoolVerdict::kReady) {
        e.slot = -1;
        free_.push_front(s);  // the next job takes the slot this one grew
        in_use_--;
        cv_work_.notify_all();
        cv_slot_.notify_all();
      }
      e.state = kDone;
      cv_done_.notify_all();
    }
  }

  Work work_;
  MakeSlot make_slot_;
  FreeSlot free_slot_;
  mutable std::mutex mu_;  // everything below
  std::condition_variable cv_work_, cv_done_, cv_slot_;
  std::deque<Entry> q_;  // pushed and not yet taken, in push order; the first started_ have a thread
  size_t started_ = 0;
  std::vector<Slot*> slots_;
  std::deque<long> free_;
  uint32_t in_use_ = 0;
  bool stopping_ = true;
  std::vector<std::thread> threads_;
  PreflightPoolStats stats_;
};

}  // namespace r0
