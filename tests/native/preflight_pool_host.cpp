// Drives risc0_amd/csrc/preflight_pool.h on the CPU as the worker does, with a fake work function
// and malloc-backed slots: a producer pushes jobs in ticket order, a consumer (the uploader) takes
// them in that order while holding one of in_flight + 1 sets, releaser threads (the provers) read
// the slot, give it back and free the set. Some jobs fail, some are left to the consumer, the
// durations are random and short. Checked: every job is consumed exactly once and in order, with
// its own verdict, message and slot contents; a held slot is never rewritten; the slots in use
// never exceed n + in_flight + 1; every thread is joined and every slot freed.
//   c++ -std=c++17 -O1 -g -pthread -I risc0_amd/csrc tests/native/preflight_pool_host.cpp
// (also with -fsanitize=thread and with -fsanitize=address,undefined). Exit status 0 and a last
// line "ok: ..." on success; the first failed check prints its line and exits 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "preflight_pool.h"

namespace {

#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
      std::exit(1);                                             \
    }                                                           \
  } while (0)

enum Mode { kGood, kFail, kLeave };

struct Job {
  int id = 0;
  Mode mode = kGood;
  unsigned work_us = 0, hold_us = 0;
  size_t words = 0;
  std::atomic<int> ran{0}, consumed{0}, released{0};
};

struct Slot {
  uint32_t* p = nullptr;
  size_t words = 0;
  std::atomic<uint64_t> bytes{0};
};

std::atomic<long> g_live_slots{0}, g_live_allocs{0};

Slot* make_slot() {
  g_live_slots++;
  return new Slot;
}
void free_slot(Slot* s) {
  if (s->p) {
    std::free(s->p);
    g_live_allocs--;
  }
  delete s;
  g_live_slots--;
}

uint32_t pattern(int id, size_t i) { return uint32_t(id) * 2654435761u + uint32_t(i) * 40503u + 1u; }

struct Rig {
  using Pool = r0::PreflightPool<Job, Slot>;
  uint32_t in_flight;
  std::atomic<long> in_use{0}, peak{0};
  Pool pool;
  // the consumer's sets and the hand-over to the releasers
  std::mutex mu;
  std::condition_variable cv;
  long free_sets;
  std::deque<std::pair<Job*, long>> ready;  // job, slot
  bool done = false;
  std::vector<std::thread> releasers;

  explicit Rig(uint32_t k)
      : in_flight(k),
        pool([this](Job* j, Slot& s, std::string* msg) { return work(j, s, msg); }, make_slot, free_slot),
        free_sets(long(k) + 1) {
    for (uint32_t t = 0; t < k; t++) releasers.emplace_back([this] { run_releaser(); });
  }

  void note_use(long d) {
    const long now = in_use.fetch_add(d) + d;
    long p = peak.load();
    while (now > p && !peak.compare_exchange_weak(p, now)) {
    }
  }

  r0::PoolVerdict work(Job* j, Slot& s, std::string* msg) {
    note_use(1);
    CHECK(j->ran.fetch_add(1) == 0, "job %d ran twice", j->id);
    if (j->mode == kLeave) {
      note_use(-1);
      return r0::PoolVerdict::kLeft;
    }
    if (j->words > s.words) {
      if (s.p) std::free(s.p);
      else g_live_allocs++;
      s.p = static_cast<uint32_t*>(std::malloc(j->words * 4));
      s.words = j->words;
      s.bytes.store(s.words * 4);
    }
    for (size_t i = 0; i < j->words; i++) s.p[i] = pattern(j->id, i);
    std::this_thread::sleep_for(std::chrono::microseconds(j->work_us));
    if (j->mode == kFail) {
      *msg = "job " + std::to_string(j->id) + " failed";
      note_use(-1);
      if (j->id % 2) throw std::runtime_error(*msg);  // both ways a work function can fail
      return r0::PoolVerdict::kFailed;
    }
    return r0::PoolVerdict::kReady;
  }

  static void check_slot(const Job* j, const Slot& s) {
    CHECK(s.words >= j->words, "job %d: slot of %zu words", j->id, s.words);
    for (size_t i = 0; i < j->words; i++)
      CHECK(s.p[i] == pattern(j->id, i), "job %d: word %zu of its slot was rewritten", j->id, i);
  }

  void run_releaser() {
    for (;;) {
      std::pair<Job*, long> item;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready.empty() || done; });
        if (ready.empty()) return;
        item = ready.front();
        ready.pop_front();
      }
      Job* j = item.first;
      if (item.second >= 0) {
        std::this_thread::sleep_for(std::chrono::microseconds(j->hold_us));
        check_slot(j, pool.slot(item.second));
        CHECK(j->released.fetch_add(1) == 0, "job %d released twice", j->id);
        note_use(-1);
        pool.release(item.second);
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        free_sets++;
      }
      cv.notify_all();
    }
  }

  // the consumer: jobs[first .. first + count) in order, each with a set
  void consume(std::vector<std::unique_ptr<Job>>& jobs, const std::vector<bool>& pooled) {
    for (size_t i = 0; i < jobs.size(); i++) {
      Job* j = jobs[i].get();
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return free_sets > 0; });
        free_sets--;
      }
      long slot = -1;
      if (pooled[i]) {
        Pool::Taken t = pool.take(j);
        CHECK(j->ran.load() == 1, "job %d was handed over before it ran", j->id);
        if (j->mode == kGood) {
          CHECK(t.verdict == r0::PoolVerdict::kReady && t.slot >= 0 && t.error.empty(), "job %d: verdict %d", j->id,
                int(t.verdict));
          check_slot(j, pool.slot(t.slot));
          slot = t.slot;
        } else if (j->mode == kFail) {
          CHECK(t.verdict == r0::PoolVerdict::kFailed && t.slot < 0, "job %d: verdict %d", j->id, int(t.verdict));
          CHECK(t.error == "job " + std::to_string(j->id) + " failed", "job %d got the message '%s'", j->id,
                t.error.c_str());
        } else {
          CHECK(t.verdict == r0::PoolVerdict::kLeft && t.slot < 0 && t.error.empty(), "job %d: verdict %d", j->id,
                int(t.verdict));
        }
      } else {
        CHECK(j->ran.load() == 0, "job %d ran on a pool that did not accept it", j->id);
      }
      CHECK(j->consumed.fetch_add(1) == 0, "job %d consumed twice", j->id);
      {
        std::lock_guard<std::mutex> lk(mu);
        ready.emplace_back(j, slot);
      }
      cv.notify_all();
    }
  }

  void wait_sets_free() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return free_sets == long(in_flight) + 1 && ready.empty(); });
  }

  void finish() {
    {
      std::lock_guard<std::mutex> lk(mu);
      done = true;
    }
    cv.notify_all();
    for (auto& t : releasers) t.join();
    releasers.clear();
  }
};

std::vector<std::unique_ptr<Job>> make_jobs(std::mt19937& rng, int count, int first_id) {
  std::vector<std::unique_ptr<Job>> jobs;
  for (int i = 0; i < count; i++) {
    auto j = std::make_unique<Job>();
    j->id = first_id + i;
    const unsigned r = rng() % 10;
    j->mode = r == 0 ? kFail : r == 1 ? kLeave : kGood;
    j->work_us = rng() % 300;
    j->hold_us = rng() % 300;
    j->words = 1 + rng() % 4096;
    jobs.push_back(std::move(j));
  }
  return jobs;
}

// one batch on a pool of n threads: push everything at once, consume in order; stop_early stops
// the pool from this thread while jobs are still queued
void batch(Rig& rig, uint32_t n, std::mt19937& rng, int count, int first_id, bool stop_early) {
  auto jobs = make_jobs(rng, count, first_id);
  std::vector<bool> pooled(jobs.size());
  for (size_t i = 0; i < jobs.size(); i++) pooled[i] = rig.pool.push(jobs[i].get());
  for (size_t i = 0; i < jobs.size(); i++) CHECK(pooled[i] == (n > 0), "push %zu on a pool of %u", i, n);
  std::thread consumer([&] { rig.consume(jobs, pooled); });
  if (stop_early) {
    rig.pool.stop();  // returns once the queue is run, the threads joined, every slot back and freed
    CHECK(rig.pool.idle(), "stop returned with jobs queued");
    CHECK(g_live_slots.load() == 0 && g_live_allocs.load() == 0, "stop left %ld slots", g_live_slots.load());
    Job late;
    CHECK(!rig.pool.push(&late), "a stopped pool accepted a job");
  }
  consumer.join();
  rig.wait_sets_free();
  for (auto& j : jobs) {
    CHECK(j->consumed.load() == 1, "job %d consumed %d times", j->id, j->consumed.load());
    CHECK(j->ran.load() == (n > 0 ? 1 : 0), "job %d ran %d times", j->id, j->ran.load());
    CHECK(j->released.load() == (n > 0 && j->mode == kGood ? 1 : 0), "job %d released %d times", j->id,
          j->released.load());
  }
  CHECK(rig.pool.idle(), "jobs left in the pool's queue");
  CHECK(rig.in_use.load() == 0, "%ld slots in use after the batch", rig.in_use.load());
}

void check_bound(Rig& rig, uint32_t n) {
  uint64_t bytes = 0;
  const r0::PreflightPoolStats st = rig.pool.stats([&](const Slot& s) { bytes += s.bytes.load(); });
  const long bound = n ? long(n) + rig.in_flight + 1 : 0;
  CHECK(st.threads == n && long(st.slots) == bound, "pool of %u: %u threads, %u slots", n, st.threads, st.slots);
  CHECK(long(st.peak_slots_in_use) <= bound, "peak %u above %ld slots", st.peak_slots_in_use, bound);
  CHECK(rig.peak.load() <= bound, "%ld slots in use at once, above %ld", rig.peak.load(), bound);
  CHECK(g_live_slots.load() == bound, "%ld slots alive, %ld expected", g_live_slots.load(), bound);
  CHECK(bytes <= uint64_t(bound) * 4096 * 4, "slot bytes %llu", (unsigned long long)bytes);
  rig.peak.store(0);
}

}  // namespace

int main() {
  int scenarios = 0;
  uint64_t total_jobs = 0;
  for (uint32_t n : {1u, 2u, 3u, 8u})
    for (uint32_t k : {1u, 3u})
      for (int count : {0, 1, 200})
        for (int stop_early = 0; stop_early < 2; stop_early++) {
          std::mt19937 rng(1000 * n + 100 * k + count + stop_early);
          {
            Rig rig(k);
            rig.pool.resize(n, k);
            batch(rig, n, rng, count, 0, stop_early != 0);
            if (!stop_early) check_bound(rig, n);
            const r0::PreflightPoolStats st = rig.pool.stats([](const Slot&) {});
            CHECK(st.jobs + st.left == uint64_t(count), "%llu + %llu jobs counted of %d",
                  (unsigned long long)st.jobs, (unsigned long long)st.left, count);
            rig.finish();
          }  // the pool's destructor stops it
          CHECK(g_live_slots.load() == 0 && g_live_allocs.load() == 0, "%ld slots, %ld buffers not freed",
                g_live_slots.load(), g_live_allocs.load());
          scenarios++;
          total_jobs += uint64_t(count);
        }
  // resize between batches, through 0 and back, on one pool
  for (uint32_t k : {1u, 3u}) {
    std::mt19937 rng(77 + k);
    Rig rig(k);
    int id = 0;
    uint64_t expect = 0;
    for (uint32_t n : {2u, 3u, 0u, 1u, 8u, 0u}) {
      rig.pool.resize(n, k);
      batch(rig, n, rng, 60, id, false);
      check_bound(rig, n);
      id += 60;
      if (n) expect += 60;
      const r0::PreflightPoolStats st = rig.pool.stats([](const Slot&) {});
      CHECK(st.jobs + st.left == expect, "the counters run on across a resize");
      total_jobs += 60;
    }
    rig.finish();
    rig.pool.stop();
    CHECK(g_live_slots.load() == 0 && g_live_allocs.load() == 0, "%ld slots, %ld buffers not freed",
          g_live_slots.load(), g_live_allocs.load());
    scenarios++;
  }
  std::printf("ok: %d scenarios, %llu jobs\n", scenarios, (unsigned long long)total_jobs);
  return 0;
}
