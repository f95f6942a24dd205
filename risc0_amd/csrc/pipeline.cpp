// Segment pipeline: many segments through one GPU with the witness upload of the next
// segment overlapped with the proofs in flight — the queue r0vm's GPU worker keeps
// (GPU_QUEUE_DEPTH=2, risc0/r0vm/src/actors/worker.rs:75-76) and the per-segment loop of
// the zkvm prover (risc0/zkvm/src/host/server/prove/prover_impl.rs:84-94), native here.
//
// One uploader thread copies a job's witness groups from host memory (page-locked for
// full PCIe rate) into a free device buffer set on its own stream, recording an event per
// group; `in_flight` prover threads each take a set as soon as its copies are queued, run
// the whole-segment prover on their own stream (which waits on each group's event just
// before that group's first use)
// (runtime.cpp gives every host thread its own stream, pool and staging), write the
// seal, and hand the set back. in_flight + 1 sets circulate, so an upload is always
// running ahead while the GPU proves. Each job reports its own error.
//
// r0hip_prove_segments and r0hip_prove_trace_segments take every job up front and return when
// all are proved; the worker (r0hip_worker_*, below) keeps the trace pipeline's threads and sets
// alive between jobs and takes rv32im jobs of any po2 and recursion jobs as they arrive.
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <functional>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/r0hip.h"
#include "backs.h"
#include "circuit.h"
#include "devmem.h"
#include "preflight_pool.h"
#include "runtime.h"

namespace r0 {
std::vector<uint32_t> prove_segment(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                    const uint32_t* data, const uint32_t* accum, uint32_t* global,
                                    bool write_version, uint32_t version, std::vector<uint32_t>* mix_out,
                                    const UploadGate* uploads, const AccumStep* acc = nullptr,
                                    GroupWork* code_early = nullptr, const CachedGroup* code_cached = nullptr);
// api.cpp: rv32im prove_core from a preflight trace, and the host check of an injector
std::vector<uint32_t> prove_trace(int suite, uint32_t po2, uint32_t mode, const uint32_t* global_in,
                                  const uint32_t* inj_index, size_t inj_rows, const uint32_t* inj_offsets,
                                  const uint32_t* inj_values, const r0hip_raw_preflight_trace* pf,
                                  const r0hip_bigint_back* h_bigint, size_t n_bigint, bool resident,
                                  std::vector<uint32_t>* mix, const std::function<void(hipStream_t)>& inputs_ready,
                                  const TraceBacks* backs);
void check_injector(const uint32_t* index, size_t rows, const uint32_t* offsets, const uint32_t* values,
                    size_t limit, size_t seg_rows);

namespace {

// Columns per upload chunk: a multiple of 16, so the prover can hash a group's rows range by
// range as the chunks land (hash_rows_range); ~200 MB per chunk at po2=20.
constexpr size_t kChunkCols = 48;

// A device buffer set and its upload state. hipMemcpyAsync from page-locked memory returns
// only when a large copy is done, so the set is handed to a prover before its copies are
// queued: the prover blocks in wait() until the uploader has queued the chunks it needs and
// recorded the last one's event, then its stream waits on that event.
struct BufSet final : UploadGate {
  DevBuf g[4];                     // code, data, accum, global
  size_t cols[4] = {1, 1, 1, 1};   // columns per group (global: one)
  size_t col_words[4] = {0, 0, 0, 0};
  std::vector<hipEvent_t> ev[4];   // per chunk, recorded on the uploader stream
  size_t job = 0;
  mutable std::mutex mu;
  mutable std::condition_variable cv;
  size_t queued[4] = {0, 0, 0, 0};  // chunks queued per group (all of them after an upload error)
  size_t chunks(int grp) const { return (cols[grp] + kChunkCols - 1) / kChunkCols; }
  size_t chunk_cols(int) const override { return kChunkCols; }
  void mark(int grp, size_t n) {
    {
      std::lock_guard<std::mutex> lk(mu);
      queued[grp] = n;
    }
    cv.notify_all();
  }
  void mark_all() {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (int i = 0; i < 4; i++) queued[i] = chunks(i);
    }
    cv.notify_all();
  }
  void wait(int grp, size_t col_end, hipStream_t s) const override {
    const size_t need = (std::min(col_end, cols[grp]) + kChunkCols - 1) / kChunkCols;
    if (need == 0) return;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return queued[grp] >= need; });
    }
    // one stream carries every copy in order: the last needed chunk's event covers the rest
    HIP_OK(hipStreamWaitEvent(s, ev[grp][need - 1], 0));
  }
};

// a bounded queue of set indices
struct Queue {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<long> q;
  void put(long v) {
    {
      std::lock_guard<std::mutex> lk(mu);
      q.push_back(v);
    }
    cv.notify_one();
  }
  long get() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return !q.empty(); });
    long v = q.front();
    q.pop_front();
    return v;
  }
};

// k provers: k - 1 threads and the calling thread, whose stream the process already holds, so
// a call keeps k + 1 streams busy (the uploader's and the provers') and the runtime's default 4
// hardware queues give each its own for k <= 3 (a shared queue runs its streams' kernels in
// order). R0_PIPE_CALLER_PROVES=0: k prover threads (the calling thread only waits).
template <typename F>
void run_provers(size_t k, F& prover) {
  static const bool caller = [] {
    const char* e = getenv("R0_PIPE_CALLER_PROVES");
    return !e || strtoul(e, nullptr, 10) != 0;
  }();
  std::vector<std::thread> threads;
  for (size_t t = caller ? 1 : 0; t < k; t++) threads.emplace_back(prover);
  if (caller) {
    // the other provers fill the chip: the calling thread proves on one stream like them,
    // whatever its r0hip_set_proof_streams setting, which it keeps
    const uint32_t streams = proof_streams();
    set_proof_streams(1);
    prover();  // returns at its stop token; never throws (errors are per job)
    set_proof_streams(streams);
  }
  for (auto& t : threads) t.join();
}

char* dup_msg(const char* m) {
  size_t n = strlen(m) + 1;
  char* p = static_cast<char*>(malloc(n));
  if (p) memcpy(p, m, n);
  return p;
}

// A device trace set: one job's preflight trace, injector and global vector, and the event
// that marks their upload on the uploader's stream. `landed`: the uploader has queued every
// copy and recorded the event, or failed (the job then carries the error).
struct TraceSet {
  DevBuf glob, index, offsets, values, cycles, txns, bigint;
  hipEvent_t ev = nullptr;
  size_t job = 0;
  std::mutex mu;
  std::condition_variable cv;
  bool landed = false;
  void mark() {
    {
      std::lock_guard<std::mutex> lk(mu);
      landed = true;
    }
    cv.notify_all();
  }
  void wait_landed() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return landed; });
  }
};

constexpr size_t kCycleWords = 9, kTxnWords = 5, kGlobalWords = 90;  // RawPreflightCycle 36 B, txn 20 B

// The host checks of one trace job (n = 2^po2); throws the job's error.
void check_trace_input(const r0hip_trace_input& t, const r0hip_bigint_back* h_bigint, size_t n_bigint, size_t n) {
  const r0hip_raw_preflight_trace& pf = t.preflight;
  R0_REQUIRE(t.h_global && t.h_inj_index && pf.cycles, "trace job: null argument");
  R0_REQUIRE(t.inj_rows <= n, "trace job: injector longer than the segment");
  R0_REQUIRE((pf.txns_len == 0 || pf.txns) && (pf.bigint_bytes_len == 0 || pf.bigint_bytes),
             "trace job: null trace array with a nonzero count");
  R0_REQUIRE(n_bigint == 0 || h_bigint, "trace job: h_bigint is NULL with n_bigint > 0");
  check_injector(t.h_inj_index, t.inj_rows, t.h_inj_offsets, t.h_inj_values, size_t(211) * n, n);
}

// The uploader's copies of one checked trace job: the trace, the injector and the global vector
// into set b on the uploader's stream, then b.ev recorded. The set's buffers hold the job (the
// callers size them).
void upload_trace(TraceSet& b, const r0hip_trace_input& t, size_t n) {
  const r0hip_raw_preflight_trace& pf = t.preflight;
  const size_t n_inj = t.h_inj_index[t.inj_rows];
  stage_reset();  // the previous job's staged copies have landed: the arena is free
  upload_async(b.glob.p, t.h_global, kGlobalWords * 4);
  upload_async(b.index.p, t.h_inj_index, (t.inj_rows + 1) * 4);
  upload_async(b.offsets.p, t.h_inj_offsets, n_inj * 4);
  upload_async(b.values.p, t.h_inj_values, n_inj * 4);
  upload_async(b.cycles.p, pf.cycles, n * kCycleWords * 4);
  upload_async(b.txns.p, pf.txns, size_t(pf.txns_len) * kTxnWords * 4);
  upload_async(b.bigint.p, pf.bigint_bytes, pf.bigint_bytes_len);
  HIP_OK(hipEventRecord(b.ev, stream()));
}

// The prover's part: prove_trace from the set's device copies. Its stream waits for the set's
// upload just before the first read of an input; *error (written by the uploader under b.mu)
// is the job's staging error, rethrown here.
// backs: the set holds the injector as Back records (a worker's kind-2 job) and not the CSR arrays
std::vector<uint32_t> prove_staged_trace(TraceSet& b, int suite, uint32_t po2, const r0hip_trace_input& tr,
                                         const r0hip_bigint_back* h_bigint, size_t n_bigint,
                                         const char* const* error, std::vector<uint32_t>* mix,
                                         const TraceBacks* backs = nullptr) {
  r0hip_raw_preflight_trace pf = tr.preflight;  // the set's device copies
  pf.cycles = b.cycles.p;
  pf.txns = pf.txns_len ? b.txns.p : nullptr;
  pf.bigint_bytes = pf.bigint_bytes_len ? reinterpret_cast<const uint8_t*>(b.bigint.p) : nullptr;
  return prove_trace(suite, po2, tr.mode, b.glob.p, b.index.p, tr.inj_rows, b.offsets.p, b.values.p, &pf, h_bigint,
                     n_bigint, true, mix, [&](hipStream_t st) {
                       b.wait_landed();
                       {
                         std::lock_guard<std::mutex> lk(b.mu);
                         if (*error) throw std::runtime_error(*error);
                       }
                       HIP_OK(hipStreamWaitEvent(st, b.ev, 0));
                     }, backs);
}

// The null checks of a kind-2 worker job's trace (n = 2^po2); its records are check_backs's.
void check_backs_trace(const r0hip_trace_input& t, const std::string& who) {
  const r0hip_raw_preflight_trace& pf = t.preflight;
  R0_REQUIRE(t.h_global && pf.cycles, who + ": trace job: null argument");
  R0_REQUIRE((pf.txns_len == 0 || pf.txns) && (pf.bigint_bytes_len == 0 || pf.bigint_bytes),
             who + ": trace job: null trace array with a nonzero count");
}

// The verifier threads' receipt check: r0hip_verify_seal, or with verify ==
// R0HIP_VERIFY_RECEIPTS_DEVICE the same check with the seal's openings hashed on the device.
const char* check_receipt(int verify, const char* circuit, int suite, const std::vector<uint32_t>& seal,
                          const uint32_t* roots, size_t n_roots, uint32_t* po2) {
  if (verify == R0HIP_VERIFY_RECEIPTS_DEVICE)
    return r0hip_verify_seal_on(R0HIP_VERIFY_DEVICE, circuit, suite, seal.data(), seal.size(), roots, n_roots, nullptr,
                                po2);
  return r0hip_verify_seal(circuit, suite, seal.data(), seal.size(), roots, n_roots, nullptr, po2);
}

// Trace jobs: the uploader copies job i's trace into a free trace set and hands the set to a
// prover at once; the prover allocates its witness groups and queues their fill (which reads no
// input), then waits on the host until the uploader has queued the set's copies and makes its
// stream wait for the set's event before the injector pass (prove_trace's inputs_ready), so the
// copies of one segment overlap the proofs of the others. k + 1 sets, sized once for the largest
// job.
// verify: each finished seal is checked by r0hip_verify_seal (the validity equation included) on
// a host thread of its own while the GPU proves the next segments, as ProverImpl::
// prove_segment_core verifies a receipt before it returns it (zkvm/src/host/server/prove/
// prover_impl.rs:262-280); a seal that fails fails its job. verify == R0HIP_VERIFY_RECEIPTS_DEVICE:
// the same check with the openings hashed on the device (check_receipt), on the verifier thread's
// own stream, which it gets the thread-local way at its first seal.
const char* prove_trace_jobs(int suite, uint32_t po2, r0hip_trace_job* jobs, size_t njobs, size_t k, int verify) {
  const size_t n = size_t(1) << po2;
  size_t cap_inj = 1, cap_txn = 1, cap_big = 4;
  for (size_t i = 0; i < njobs; i++) {
    const r0hip_trace_input* t = &jobs[i].trace;
    if (t->h_inj_index && t->inj_rows <= n) cap_inj = std::max<size_t>(cap_inj, t->h_inj_index[t->inj_rows]);
    cap_txn = std::max<size_t>(cap_txn, t->preflight.txns_len);
    cap_big = std::max<size_t>(cap_big, t->preflight.bigint_bytes_len);
  }
  std::vector<TraceSet> sets(k + 1);
  struct Events {
    std::vector<TraceSet>& sets;
    ~Events() {
      for (auto& s : sets)
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
  } events{sets};
  for (auto& s : sets) {
    s.glob = DevBuf(kGlobalWords);
    s.index = DevBuf(n + 1);
    s.offsets = DevBuf(cap_inj);
    s.values = DevBuf(cap_inj);
    s.cycles = DevBuf(n * kCycleWords);
    s.txns = DevBuf(cap_txn * kTxnWords);
    s.bigint = DevBuf((cap_big + 3) / 4);
    HIP_OK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  }
  HIP_OK(hipDeviceSynchronize());  // allocations complete before other streams use them
  Queue free_q, ready_q;
  for (size_t s = 0; s < sets.size(); s++) free_q.put(long(s));

  std::thread uploader([&] {
    for (size_t i = 0; i < njobs; i++) {
      long s = free_q.get();
      TraceSet& b = sets[s];
      {
        std::lock_guard<std::mutex> lk(b.mu);
        b.job = i;
        b.landed = false;
      }
      ready_q.put(s);  // the prover fills its groups while the trace uploads
      try {
        ensure_init();
        check_trace_input(jobs[i].trace, jobs[i].h_bigint, jobs[i].n_bigint, n);
        upload_trace(b, jobs[i].trace, n);
      } catch (const std::exception& e) {
        {
          std::lock_guard<std::mutex> lk(b.mu);
          if (!jobs[i].error) jobs[i].error = dup_msg(e.what());
        }
        drain_after_error();
      }
      b.mark();
    }
    // every copy done before the call returns: the caller may free its host buffers then
    drain_after_error();
    for (size_t t = 0; t < k; t++) ready_q.put(-1);
  });

  // the receipt check: finished seals queue here (job index and seal) for the verifier thread
  std::mutex vmu;
  std::condition_variable vcv;
  std::deque<std::pair<long, std::vector<uint32_t>>> vq;
  std::thread verifier;
  if (verify)
    verifier = std::thread([&] {
      for (;;) {
        std::pair<long, std::vector<uint32_t>> item;
        {
          std::unique_lock<std::mutex> lk(vmu);
          vcv.wait(lk, [&] { return !vq.empty(); });
          item = std::move(vq.front());
          vq.pop_front();
        }
        if (item.first < 0) return;
        r0hip_trace_job& j = jobs[item.first];
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t got = 0;
        const char* err = check_receipt(verify, "rv32im", suite, item.second, nullptr, 0, &got);
        j.verify_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!err && got != po2) err = dup_msg("the seal is of another segment size");
        std::lock_guard<std::mutex> lk(vmu);
        if (err) {
          if (!j.error) j.error = dup_msg((std::string("receipt verification failed: ") + err).c_str());
          free(const_cast<char*>(err));
        } else {
          j.verified = 1;
        }
      }
    });
  auto to_verifier = [&](long job, std::vector<uint32_t> seal) {
    {
      std::lock_guard<std::mutex> lk(vmu);
      vq.emplace_back(job, std::move(seal));
    }
    vcv.notify_one();
  };

  const long corrupt_job = [] {
    const char* e = getenv("R0HIP_TESTING_CORRUPT_SEAL_JOB");
    return e ? strtol(e, nullptr, 10) : -1L;
  }();
  auto prover = [&] {
    for (;;) {
      long s = ready_q.get();
      if (s < 0) return;
      TraceSet& b = sets[s];
      const long job = long(b.job);
      r0hip_trace_job& j = jobs[job];
      const r0hip_trace_input& tr = j.trace;
      const auto t0 = std::chrono::steady_clock::now();
      try {
        ensure_init();
        std::vector<uint32_t> mix;
        std::vector<uint32_t> seal = prove_staged_trace(b, suite, po2, tr, j.h_bigint, j.n_bigint, &j.error, &mix);
        HIP_OK(hipStreamSynchronize(stream()));
        j.prove_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        j.seal_len = seal.size();
        if (j.h_mix_out) memcpy(j.h_mix_out, mix.data(), mix.size() * 4);
        // TESTING ONLY (tests/test_rv32im_witgen_gpu.py): R0HIP_TESTING_CORRUPT_SEAL_JOB=i flips a
        // bit of job i's first Merkle root word, so its receipt check must fail that job alone
        if (job == corrupt_job && seal.size() > 92) seal[92] ^= 1u;
        R0_REQUIRE(!j.h_seal || seal.size() <= j.seal_cap, "seal buffer too small");
        if (j.h_seal) memcpy(j.h_seal, seal.data(), seal.size() * 4);
        if (verify) to_verifier(job, std::move(seal));
      } catch (const std::exception& e) {
        {
          std::lock_guard<std::mutex> lk(b.mu);
          if (!j.error) j.error = dup_msg(e.what());
        }
        drain_after_error();  // kernels queued before the throw may still read this set
      }
      b.wait_landed();  // the uploader is done with this job before the set is refilled
      free_q.put(s);
    }
  };
  run_provers(k, prover);
  uploader.join();
  if (verify) {
    to_verifier(-1, {});
    verifier.join();
  }
  for (size_t i = 0; i < njobs; i++)
    if (jobs[i].error) return dup_msg((std::string("segment ") + std::to_string(i) + ": " + jobs[i].error).c_str());
  return nullptr;
}


// ---- the worker: a persistent queue of mixed jobs (r0hip_worker_*) ----------------------------
// The threads and sets of prove_trace_jobs kept alive between jobs: the uploader takes jobs from
// a FIFO in ticket order, stages each into a free set and hands the set to a prover at once; a
// prover's stream waits on the set's event before the first read of a staged input; finished
// seals go to the verifier thread (or straight to the finished list) and r0hip_worker_wait
// hands them out in completion order. The trace buffers of a set are sized for max_po2; the
// injector, transaction, BigInt and control-group buffers grow on the uploader thread while the
// set is free, before the set is handed to a prover (which reads their pointers then). A job of
// kind R0HIP_JOB_RECURSION_PROGRAM stages nothing and grows nothing: its control group and the
// group's commitment live in the caller's handle, on which the job holds a use count from
// submit to finish().
// page-locked host words that grow (a kind-4 job's preflight is written here by the uploader and
// copied to the device by the set's prover without staging)
struct PinnedWords {
  uint32_t* p = nullptr;
  size_t words = 0;
  PinnedWords() = default;
  PinnedWords(const PinnedWords&) = delete;
  PinnedWords& operator=(const PinnedWords&) = delete;
  PinnedWords(PinnedWords&& o) noexcept : p(o.p), words(o.words) { o.p = nullptr, o.words = 0; }
  ~PinnedWords() {
    if (p) (void)hipHostFree(p);
  }
  void reserve(size_t n, unsigned flags = hipHostMallocDefault) {
    if (n <= words) return;
    if (p) (void)hipHostFree(p);
    p = nullptr, words = 0;
    void* q = nullptr;
    HIP_OK(hipHostMalloc(&q, n * 4, flags));
    p = static_cast<uint32_t*>(q), words = n;
  }
};

// one slot of the worker's preflight pool (preflight_pool.h): what a set holds for a kind-4 job,
// owned by the pool so a preflight can run before its job has a set. `bytes` is what get_stats
// reads while a pool thread grows the slot.
struct PfSlot {
  PinnedWords wom, iops;
  std::vector<uint32_t> out;
  std::atomic<uint64_t> bytes{0};
};

struct WorkerSet : TraceSet {
  DevBuf ctrl;  // recursion jobs: the control group (allocated at the set's first one)
  PinnedWords pf_wom, pf_iops;  // kind-4 jobs: the preflight's WOM and IOP values
  std::vector<uint32_t> pf_out;
  // where wjob's preflight is: the set's own buffers above (the uploader ran it) or those of the
  // pool's slot pf_slot, which the prover gives back once its stream has drained
  const uint32_t *pf_wom_p = nullptr, *pf_iops_p = nullptr;
  long pf_slot = -1;
  r0hip_worker_job* wjob = nullptr;
  bool witness_check = false;  // wjob's r0hip_worker_set_witness_check mode, as recorded at its submit
  size_t cap_inj = 0, cap_txn = 0, cap_big = 0;  // entries, records, bytes
  // kind-2 jobs: the Back records and their payload words (allocated at the set's first one),
  // the counts of the uploader's check and the BigInt records it derived for the accumulation
  DevBuf recs, words;
  size_t cap_recs = 0, cap_words = 0;
  BacksInfo backs_info;
  std::vector<r0hip_bigint_back> backs_bigint;
};

// a job of kind R0HIP_JOB_RECURSION_PROGRAM is the first member of an r0hip_worker_program_job,
// one of kind R0HIP_JOB_RECURSION_INPUT of an r0hip_worker_input_job: the handle follows the job
static_assert(offsetof(r0hip_worker_input_job, program) == offsetof(r0hip_worker_program_job, program),
              "the handle sits at one offset in both job structs");
inline const r0hip_recursion_program* job_program(const r0hip_worker_job* j) {
  return reinterpret_cast<const r0hip_worker_program_job*>(j)->program;
}
inline bool job_holds_program(const r0hip_worker_job* j) {
  return j->kind == R0HIP_JOB_RECURSION_PROGRAM || j->kind == R0HIP_JOB_RECURSION_INPUT;
}

struct WorkerImpl {
  uint32_t max_po2 = 0;
  size_t k = 0;
  int verify = 0;  // r0hip_worker_create's: 0 none, R0HIP_VERIFY_RECEIPTS_DEVICE device openings, else host
  uint32_t key[8] = {};
  std::vector<WorkerSet> sets;
  Queue free_q, ready_q;
  std::mutex mu;  // fifo, finished, next_ticket, outstanding, stopping
  std::condition_variable cv_in, cv_done;
  std::deque<r0hip_worker_job*> finished;
  std::deque<std::pair<r0hip_worker_job*, BacksInfo>> fifo;  // with the submit check's counts (kind 2)
  uint64_t next_ticket = 0;
  // r0hip_worker_set_witness_check: the switch, and the queued jobs submitted while it was on (a
  // job struct has no room for the mode and keeps its layout); the uploader moves a job's entry
  // to its set
  bool witness_check = false;
  std::set<const r0hip_worker_job*> checked_jobs;
  size_t outstanding = 0;
  bool stopping = false;
  std::mutex vmu;
  std::condition_variable vcv;
  std::deque<std::pair<r0hip_worker_job*, std::vector<uint32_t>>> vq;
  std::thread uploader, verifier;
  std::vector<std::thread> provers;
  // r0hip_worker_set_preflight_threads: the pool that runs kind-4 preflights ahead of the uploader
  // and the queued jobs it was given at submit (under mu, as checked_jobs); the uploader's own
  // counters for r0hip_worker_get_stats
  using PfPool = PreflightPool<r0hip_worker_job, PfSlot>;
  PfPool pool{pool_preflight, [] { return new PfSlot; }, [](PfSlot* s) { delete s; }};
  std::set<const r0hip_worker_job*> pooled_jobs;
  std::mutex stats_mu;
  uint64_t inline_jobs = 0;
  double uploader_preflight_ms = 0, uploader_wait_preflight_ms = 0;

  // a kind-4 job's preflight, into (wom, iops, out); the job's output fields are written here
  static void preflight_job(r0hip_worker_job* j, const RecursionInputCounts& cnt, PinnedWords& wom, PinnedWords& iops,
                            std::vector<uint32_t>& out, unsigned host_flags) {
    auto* ij = reinterpret_cast<r0hip_worker_input_job*>(j);
    ij->n_output = cnt.n_output;
    R0_REQUIRE(!ij->h_output || cnt.n_output <= ij->output_cap,
               "recursion input job: output buffer too small: the program writes " + std::to_string(cnt.n_output) +
                   " words");
    wom.reserve(cnt.n_wom * 4 + 4, host_flags);
    iops.reserve(cnt.n_iops * 4 + 4, host_flags);
    out.resize(cnt.n_output);
    recursion_program_preflight_into(job_program(j), ij->h_input, ij->n_input, wom.p, iops.p, out.data());
    if (ij->h_output && cnt.n_output) memcpy(ij->h_output, out.data(), cnt.n_output * 4);
  }

  // on a pool thread, which never uses the device: no ensure_init, no stream, no copy. The only
  // HIP calls are the page-locked allocation and free of the slot, portable because this thread
  // has not chosen the library's device. A handle without a plan is left to the uploader, since
  // making the plan drains the device; a failure (a throw) is the job's own.
  static PoolVerdict pool_preflight(r0hip_worker_job* j, PfSlot& s, std::string*) {
    RecursionInputCounts cnt;
    if (!recursion_program_planned_counts(job_program(j), &cnt)) return PoolVerdict::kLeft;
    struct Sized {  // also when the preflight throws after the slot grew
      PfSlot& s;
      ~Sized() { s.bytes.store((s.wom.words + s.iops.words) * 4, std::memory_order_relaxed); }
    } sized{s};
    preflight_job(j, cnt, s.wom, s.iops, s.out, hipHostMallocPortable);
    return PoolVerdict::kReady;
  }

  void finish(r0hip_worker_job* j) {
    // the job's proof has drained (or never ran): its hold on a resident program ends here,
    // before r0hip_worker_wait can hand the job back
    if (job_holds_program(j)) recursion_program_release(job_program(j));
    {
      std::lock_guard<std::mutex> lk(mu);
      finished.push_back(j);
    }
    cv_done.notify_all();
  }
  void to_verifier(r0hip_worker_job* j, std::vector<uint32_t> seal) {
    {
      std::lock_guard<std::mutex> lk(vmu);
      vq.emplace_back(j, std::move(seal));
    }
    vcv.notify_one();
  }

  // the set is free (its last prover drained its stream): make its buffers hold job j
  void grow(WorkerSet& b, const r0hip_worker_job& j, const BacksInfo& info) {
    const size_t n = size_t(1) << j.po2;
    if (j.kind == R0HIP_JOB_RECURSION) {
      if (b.ctrl.words < 23 * n) b.ctrl = DevBuf(23 * n);
      return;
    }
    if (job_holds_program(&j)) return;  // the control group lives in the handle
    const r0hip_trace_input& t = j.trace;
    if (j.kind == R0HIP_JOB_RV32IM_BACKS) {  // checked at submit: at most n records, n_words below 2^32
      if (j.backs->n > b.cap_recs) {
        b.recs = DevBuf(j.backs->n * 3);
        b.cap_recs = j.backs->n;
      }
      if (j.backs->n_words > b.cap_words) {
        b.words = DevBuf(j.backs->n_words);
        b.cap_words = j.backs->n_words;
      }
      // what the prover reads on the host: the check's counts and the accumulation's BigInt
      // records, derived from the payloads in one pass
      b.backs_info = info;
      b.backs_bigint = backs_bigint_records(*j.backs, info.n_bigint);
    } else {
      // an index that names more entries than the data group has words is refused by run_uploader
      const size_t n_inj = t.inj_rows <= n ? t.h_inj_index[t.inj_rows] : 0;
      if (n_inj > b.cap_inj && n_inj <= 211 * n) {
        b.offsets = DevBuf(n_inj);
        b.values = DevBuf(n_inj);
        b.cap_inj = n_inj;
      }
    }
    if (t.preflight.txns_len > b.cap_txn) {
      b.txns = DevBuf(size_t(t.preflight.txns_len) * kTxnWords);
      b.cap_txn = t.preflight.txns_len;
    }
    if (t.preflight.bigint_bytes_len > b.cap_big) {
      b.bigint = DevBuf((size_t(t.preflight.bigint_bytes_len) + 3) / 4);
      b.cap_big = t.preflight.bigint_bytes_len;
    }
  }

  void run_uploader() {
    for (;;) {
      r0hip_worker_job* j;
      BacksInfo info;
      bool job_check = false, job_pooled = false;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_in.wait(lk, [&] { return !fifo.empty() || stopping; });
        if (fifo.empty()) break;
        j = fifo.front().first;
        info = fifo.front().second;
        fifo.pop_front();
        job_check = checked_jobs.erase(j) != 0;
        job_pooled = pooled_jobs.erase(j) != 0;
      }
      const long s = free_q.get();
      WorkerSet& b = sets[s];
      auto fail = [&](const char* what) {
        {
          std::lock_guard<std::mutex> lk(b.mu);
          if (!j->error) j->error = dup_msg(what);
        }
        drain_after_error();
      };
      bool ok = true;
      {
        std::lock_guard<std::mutex> lk(b.mu);
        b.wjob = j;
        b.witness_check = job_check;
        b.landed = false;
      }
      try {
        ensure_init();
        grow(b, *j, info);
      } catch (const std::exception& e) {
        fail(e.what());
        ok = false;
      }
      ready_q.put(s);  // the prover fills its groups while the inputs upload
      // a job the pool was given is taken from it whatever happened above: the pool's queue is in
      // ticket order, and a finished preflight's slot goes back through the set's prover
      PfPool::Taken taken;
      if (job_pooled) try {
          const auto t0 = std::chrono::steady_clock::now();
          taken = pool.take(j);
          const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
          if (taken.verdict == PoolVerdict::kReady) b.pf_slot = taken.slot;
          std::lock_guard<std::mutex> lk(stats_mu);
          uploader_wait_preflight_ms += ms;
        } catch (const std::exception& e) {
          fail(e.what());
          ok = false;
        }
      if (ok) try {
          const size_t n = size_t(1) << j->po2;
          if (j->kind == R0HIP_JOB_RECURSION) {
            stage_reset();
            upload_async(b.ctrl.p, j->recursion.h_ctrl, 23 * n * 4);
            HIP_OK(hipEventRecord(b.ev, stream()));
          } else if (j->kind == R0HIP_JOB_RECURSION_PROGRAM) {
            // nothing to stage: the prover reads the handle and the job's host arrays
          } else if (j->kind == R0HIP_JOB_RECURSION_INPUT) {
            // the preflight, here, while the provers work: into the set's page-locked buffers,
            // which its prover copies up itself. Nothing stays queued on this thread's stream: the
            // first job of a handle makes its plan here (a read-back, the run keys and their sort),
            // and recursion_program_prepare_input drains before it returns
            // With a pool (r0hip_worker_set_preflight_threads) a pool thread has run it into a slot,
            // output and failure included, and the set is pointed at the slot; only a job whose
            // handle had no plan then is left to this thread
            if (job_pooled && taken.verdict == PoolVerdict::kReady) {
              PfSlot& slot = pool.slot(taken.slot);
              b.pf_wom_p = slot.wom.p, b.pf_iops_p = slot.iops.p;
            } else if (job_pooled && taken.verdict == PoolVerdict::kFailed) {
              throw std::runtime_error(taken.error);
            } else {
              const RecursionInputCounts cnt = recursion_program_prepare_input(job_program(j));
              struct Count {  // a failed preflight is counted too, as the pool counts its own
                WorkerImpl& m;
                std::chrono::steady_clock::time_point t0;
                ~Count() {
                  const double ms =
                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                  std::lock_guard<std::mutex> lk(m.stats_mu);
                  m.inline_jobs++;
                  m.uploader_preflight_ms += ms;
                }
              } count{*this, std::chrono::steady_clock::now()};
              preflight_job(j, cnt, b.pf_wom, b.pf_iops, b.pf_out, hipHostMallocDefault);
              b.pf_wom_p = b.pf_wom.p, b.pf_iops_p = b.pf_iops.p;
            }
          } else if (j->kind == R0HIP_JOB_RV32IM_BACKS) {
            // the records were checked at submit; no index, offsets or values are staged
            const r0hip_raw_preflight_trace& pf = j->trace.preflight;
            stage_reset();  // the previous job's staged copies have landed: the arena is free
            upload_async(b.glob.p, j->trace.h_global, kGlobalWords * 4);
            upload_async(b.recs.p, j->backs->recs, j->backs->n * sizeof(r0hip_back));
            upload_async(b.words.p, j->backs->words, j->backs->n_words * 4);
            upload_async(b.cycles.p, pf.cycles, n * kCycleWords * 4);
            upload_async(b.txns.p, pf.txns, size_t(pf.txns_len) * kTxnWords * 4);
            upload_async(b.bigint.p, pf.bigint_bytes, pf.bigint_bytes_len);
            HIP_OK(hipEventRecord(b.ev, stream()));
          } else {
            check_trace_input(j->trace, j->h_bigint, j->n_bigint, n);
            R0_REQUIRE(j->trace.h_inj_index[j->trace.inj_rows] <= b.cap_inj,
                       "trace job: the injector has more entries than the data group has words");
            upload_trace(b, j->trace, n);
          }
        } catch (const std::exception& e) {
          fail(e.what());
        }
      b.mark();
    }
    // every copy done before the threads end
    drain_after_error();
    for (size_t t = 0; t < k; t++) ready_q.put(-1);
  }

  void run_prover() {
    for (;;) {
      const long s = ready_q.get();
      if (s < 0) return;
      WorkerSet& b = sets[s];
      r0hip_worker_job* j;
      {
        std::lock_guard<std::mutex> lk(b.mu);
        j = b.wjob;
        set_witness_check_mode(b.witness_check);  // this prover thread's mode, for this job
      }
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<uint32_t> seal;
      bool ok = false;
      try {
        ensure_init();
        std::vector<uint32_t> mix;
        if (j->kind == R0HIP_JOB_RECURSION) {
          b.wait_landed();
          {
            std::lock_guard<std::mutex> lk(b.mu);
            if (j->error) throw std::runtime_error(j->error);
          }
          HIP_OK(hipStreamWaitEvent(stream(), b.ev, 0));
          const r0hip_recursion_input& in = j->recursion;
          seal = prove_recursion(j->suite, j->po2, b.ctrl.p, in.h_wom, in.n_wom, in.h_cycles, in.n_cycles, in.h_iops,
                                 in.n_iops, keyed_noise(key, j->ticket), &mix);
        } else if (j->kind == R0HIP_JOB_RECURSION_PROGRAM) {
          b.wait_landed();  // at once: the uploader stages nothing for this kind
          {
            std::lock_guard<std::mutex> lk(b.mu);
            if (j->error) throw std::runtime_error(j->error);
          }
          const r0hip_recursion_input& in = j->recursion;
          seal = prove_recursion_program(job_program(j), in.h_wom, in.n_wom, in.h_cycles, in.n_cycles, in.h_iops,
                                         in.n_iops, keyed_noise(key, j->ticket), &mix);
        } else if (j->kind == R0HIP_JOB_RECURSION_INPUT) {
          b.wait_landed();  // the uploader has run the preflight into the set's buffers
          {
            std::lock_guard<std::mutex> lk(b.mu);
            if (j->error) throw std::runtime_error(j->error);
          }
          seal = prove_recursion_program_input(job_program(j), nullptr, 0, b.pf_wom_p, b.pf_iops_p, nullptr,
                                               keyed_noise(key, j->ticket), &mix);
        } else if (j->kind == R0HIP_JOB_RV32IM_BACKS) {
          // the set's counts and BigInt records were written by the uploader before the hand-over
          // (grow); the record and word counts are the caller's, checked at submit
          const TraceBacks tb{b.recs.p, j->backs->n, b.words.p, j->backs->n_words, j->backs->inj_rows,
                              b.backs_info.entries};
          seal = prove_staged_trace(b, j->suite, j->po2, j->trace,
                                    b.backs_bigint.empty() ? nullptr : b.backs_bigint.data(), b.backs_bigint.size(),
                                    &j->error, &mix, &tb);
        } else {
          seal = prove_staged_trace(b, j->suite, j->po2, j->trace, j->h_bigint, j->n_bigint, &j->error, &mix);
        }
        HIP_OK(hipStreamSynchronize(stream()));
        j->prove_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        j->seal_len = seal.size();
        if (j->h_mix_out) memcpy(j->h_mix_out, mix.data(), mix.size() * 4);
        R0_REQUIRE(!j->h_seal || seal.size() <= j->seal_cap, "seal buffer too small");
        if (j->h_seal) memcpy(j->h_seal, seal.data(), seal.size() * 4);
        ok = true;
      } catch (const std::exception& e) {
        {
          std::lock_guard<std::mutex> lk(b.mu);
          if (!j->error) j->error = dup_msg(e.what());
        }
        drain_after_error();  // kernels queued before the throw may still read this set
      }
      b.wait_landed();  // the uploader is done with this job before the set is refilled
      if (b.pf_slot >= 0) {
        // the stream has drained on both paths above: nothing reads the slot's buffers any more
        pool.release(b.pf_slot);
        b.pf_slot = -1;
      }
      free_q.put(s);
      if (ok && verify) to_verifier(j, std::move(seal));
      else finish(j);
    }
  }

  void run_verifier() {
    for (;;) {
      std::pair<r0hip_worker_job*, std::vector<uint32_t>> item;
      {
        std::unique_lock<std::mutex> lk(vmu);
        vcv.wait(lk, [&] { return !vq.empty(); });
        item = std::move(vq.front());
        vq.pop_front();
      }
      r0hip_worker_job* j = item.first;
      if (!j) return;
      const bool rec = j->kind == R0HIP_JOB_RECURSION || job_holds_program(j);
      const auto t0 = std::chrono::steady_clock::now();
      uint32_t got = 0;
      const uint32_t* roots = rec ? j->recursion.h_code_roots : nullptr;
      size_t n_roots = rec ? j->recursion.n_code_roots : 0;
      if (job_holds_program(j) && n_roots == 0) {
        // no allow-list given: the seal must carry the handle's own control id
        roots = recursion_program_shape(job_program(j)).control_id;
        n_roots = 1;
      }
      const char* err = check_receipt(verify, rec ? "recursion" : "rv32im", j->suite, item.second, roots, n_roots, &got);
      j->verify_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (!err && got != j->po2) err = dup_msg("the seal is of another segment size");
      if (err) {
        j->error = dup_msg((std::string("receipt verification failed: ") + err).c_str());
        free(const_cast<char*>(err));
      } else {
        j->verified = 1;
      }
      finish(j);
    }
  }

  // runs everything submitted to completion, joins the threads, frees the sets
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stopping = true;
    }
    cv_in.notify_all();
    if (uploader.joinable()) uploader.join();
    else
      for (size_t t = 0; t < provers.size(); t++) ready_q.put(-1);  // create failed before the uploader
    for (auto& t : provers) t.join();
    if (verifier.joinable()) {
      to_verifier(nullptr, {});
      verifier.join();
    }
    pool.stop();  // idle: every job was taken and every slot given back before the threads above ended
    for (auto& b : sets)
      if (b.ev) (void)hipEventDestroy(b.ev);
    sets.clear();
    explicit_bzero(key, sizeof key);
  }
};

}  // namespace
}  // namespace r0

using namespace r0;

namespace {
const char* prove_segments_impl(const char* circuit, int suite, uint32_t po2, int write_version, uint32_t version,
                                r0hip_segment_job* jobs, size_t njobs, uint32_t in_flight) {
  try {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    R0_REQUIRE(po2 >= 1 && po2 <= 24, "po2 out of range");
    R0_REQUIRE(njobs == 0 || jobs, "jobs is NULL");
    ensure_init();
    if (njobs == 0) return nullptr;
    const size_t k = std::max<size_t>(1, std::min<size_t>(in_flight ? in_flight : 2, njobs));
    for (size_t i = 0; i < njobs; i++) {
      jobs[i].error = nullptr;
      jobs[i].seal_len = 0;
    }
    const bool device_accum_ok = std::string(c->name) == "rv32im";
    const size_t n = size_t(1) << po2;
    // group_sizes: accum 0, code 1, data 2 (the reference's register-group order)
    const size_t words[4] = {c->group_sizes[1] * n, c->group_sizes[2] * n, c->group_sizes[0] * n, c->output_size};
    std::vector<BufSet> sets(k + 1);
    struct Events {  // destroyed on every exit path
      std::vector<BufSet>& sets;
      ~Events() {
        for (auto& s : sets)
          for (auto& v : s.ev)
            for (auto e : v)
              if (e) (void)hipEventDestroy(e);
      }
    } events{sets};
    const size_t gcols[4] = {c->group_sizes[1], c->group_sizes[2], c->group_sizes[0], 1};
    for (auto& s : sets)
      for (int g = 0; g < 4; g++) {
        s.g[g] = DevBuf(words[g]);
        s.cols[g] = std::max<size_t>(1, gcols[g]);
        s.col_words[g] = g == 3 ? words[3] : n;
        s.ev[g].assign(s.chunks(g), nullptr);
        for (auto& e : s.ev[g]) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      }
    HIP_OK(hipDeviceSynchronize());  // allocations complete before other streams use them
    for (size_t i = 0; i < njobs; i++) {
      jobs[i].error = nullptr;
      jobs[i].seal_len = 0;
    }

    Queue free_q, ready_q;
    for (size_t s = 0; s < sets.size(); s++) free_q.put(long(s));

    std::thread uploader([&] {
      for (size_t i = 0; i < njobs; i++) {
        long s = free_q.get();
        BufSet& b = sets[s];
        b.job = i;
        {
          std::lock_guard<std::mutex> lk(b.mu);
          for (auto& q : b.queued) q = 0;  // the set is free: no prover waits on it
        }
        const uint32_t* src[4] = {jobs[i].h_code, jobs[i].h_data, jobs[i].h_accum, jobs[i].h_global};
        // rv32im without an accum group: the prover accumulates on the device
        const bool dev_accum = !src[2] && device_accum_ok;
        bool null_group = false;
        for (int g = 0; g < 4; g++) null_group |= !src[g] && !(g == 2 && dev_accum);
        if (null_group) jobs[i].error = dup_msg("witness group pointer is NULL");  // before the hand-over
        else if (jobs[i].n_bigint && (!dev_accum || !jobs[i].h_bigint))
          // the states need the mix drawn inside the proof: only a device accumulation takes them
          jobs[i].error = dup_msg("BigInt backs given without a device accumulation (h_accum must be NULL, rv32im)");
        null_group |= jobs[i].error != nullptr;
        ready_q.put(s);  // a prover may start now; it waits per group (BufSet::wait)
        if (null_group) {
          b.mark_all();
          continue;
        }
        try {
          ensure_init();
          // in the order the prover first touches them (globals, code, data, accum), each in
          // column chunks, so a segment's commits run while its later columns still upload
          for (int g : {3, 0, 1, 2}) {
            if (g == 2 && dev_accum) {
              b.mark(g, b.chunks(g));  // nothing to upload; the prover never waits on it
              continue;
            }
            for (size_t k = 0; k < b.chunks(g); k++) {
              const size_t c0 = k * kChunkCols, cc = std::min(kChunkCols, b.cols[g] - c0);
              HIP_OK(hipMemcpyAsync(b.g[g].p + c0 * b.col_words[g], src[g] + c0 * b.col_words[g],
                                    cc * b.col_words[g] * 4, hipMemcpyHostToDevice, stream()));
              HIP_OK(hipEventRecord(b.ev[g][k], stream()));
              b.mark(g, k + 1);
            }
          }
        } catch (const std::exception& e) {
          {
            std::lock_guard<std::mutex> lk(b.mu);
            if (!jobs[i].error) jobs[i].error = dup_msg(e.what());
          }
          // the job's earlier chunks may still be copying: no prover waits on them now, and
          // the set goes back to the free queue once the prover sees the error
          drain_after_error();
          b.mark_all();  // release a waiting prover; the job reports the error
        }
      }
      // every copy done before the call can return: a prover that failed early never waited
      // on its job's events, and the caller may free its host buffers once we return (free
      // on the success path, where every event was waited on)
      drain_after_error();
      for (size_t t = 0; t < k; t++) ready_q.put(-1);  // one stop token per prover
    });

    auto prover = [&] {
      for (;;) {
        long s = ready_q.get();
        if (s < 0) return;
        BufSet& b = sets[s];
        r0hip_segment_job& j = jobs[b.job];
        // j.error is written by the uploader under b.mu while this job's copies are queued
        auto failed = [&] {
          std::lock_guard<std::mutex> lk(b.mu);
          return j.error != nullptr;
        };
        if (!failed()) {
          try {
            ensure_init();
            std::vector<uint32_t> mix;
            const bool dev_accum = !j.h_accum;  // (rv32im only: checked by the uploader)
            const AccumStep acc{b.g[2].p, n, true, j.h_bigint, j.n_bigint};
            std::vector<uint32_t> seal =
                prove_segment(*c, suite, po2, b.g[0].p, b.g[1].p, dev_accum ? nullptr : b.g[2].p, b.g[3].p,
                              write_version != 0, version, &mix, &b, dev_accum ? &acc : nullptr);
            HIP_OK(hipStreamSynchronize(stream()));
            if (!failed()) {  // an upload error leaves the proof meaningless: drop it
              j.seal_len = seal.size();
              if (j.h_mix_out) memcpy(j.h_mix_out, mix.data(), mix.size() * 4);
              R0_REQUIRE(!j.h_seal || seal.size() <= j.seal_cap, "seal buffer too small");
              if (j.h_seal) memcpy(j.h_seal, seal.data(), seal.size() * 4);
            }
          } catch (const std::exception& e) {
            {
              std::lock_guard<std::mutex> lk(b.mu);
              if (!j.error) j.error = dup_msg(e.what());
            }
            // kernels queued before the throw may still read this buffer set: drain
            // them before the uploader refills it
            drain_after_error();
          }
        }
        free_q.put(s);
      }
    };
    run_provers(k, prover);
    uploader.join();
    for (size_t i = 0; i < njobs; i++)
      if (jobs[i].error) return dup_msg((std::string("segment ") + std::to_string(i) + ": " + jobs[i].error).c_str());
    return nullptr;
  } catch (const std::exception& e) {
    return dup_msg(e.what());
  } catch (...) {
    return dup_msg("r0hip: unknown error");
  }
}
}  // namespace

extern "C" const char* r0hip_prove_segments(const char* circuit, int suite, uint32_t po2, int write_version,
                                            uint32_t version, r0hip_segment_job* jobs, size_t njobs,
                                            uint32_t in_flight) {
  const char* err = prove_segments_impl(circuit, suite, po2, write_version, version, jobs, njobs, in_flight);
  // the buffer sets are freed; the calling thread (one of the provers) keeps no device memory
  drain_after_error();
  release_thread_memory();
  return err;
}

extern "C" const char* r0hip_prove_trace_segments(int suite, uint32_t po2, r0hip_trace_job* jobs, size_t njobs,
                                                  uint32_t in_flight, int verify) {
  const char* err = nullptr;
  try {
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    R0_REQUIRE(po2 >= 2 && po2 <= 24, "po2 out of range");
    R0_REQUIRE(njobs == 0 || jobs, "jobs is NULL");
    ensure_init();
    for (size_t i = 0; i < njobs; i++) {
      jobs[i].error = nullptr;
      jobs[i].seal_len = 0;
      jobs[i].verified = 0;
      jobs[i].verify_ms = 0;
      jobs[i].prove_ms = 0;
    }
    if (njobs) {
      const size_t k = std::max<size_t>(1, std::min<size_t>(in_flight ? in_flight : 2, njobs));
      err = prove_trace_jobs(suite, po2, jobs, njobs, k, verify);
    }
  } catch (const std::exception& e) {
    err = dup_msg(e.what());
  } catch (...) {
    err = dup_msg("r0hip: unknown error");
  }
  // the trace sets are freed; the calling thread (one of the provers) keeps no device memory
  drain_after_error();
  release_thread_memory();
  return err;
}

// ---- the worker's C ABI ----
struct r0hip_worker {
  WorkerImpl impl;
};

namespace {
template <typename F>
const char* guarded(F f) {
  try {
    f();
  } catch (const std::exception& e) {
    return dup_msg(e.what());
  } catch (...) {
    return dup_msg("r0hip: unknown error");
  }
  return nullptr;
}
}  // namespace

extern "C" const char* r0hip_worker_create(r0hip_worker** out, uint32_t max_po2, uint32_t in_flight, int verify,
                                           const uint32_t* h_noise_key) {
  r0hip_worker* w = nullptr;
  const char* err = guarded([&] {
    R0_REQUIRE(out, "r0hip_worker_create: out is NULL");
    *out = nullptr;
    R0_REQUIRE(max_po2 >= 2 && max_po2 <= 24, "r0hip_worker_create: max_po2 out of range");
    R0_REQUIRE(in_flight <= 8, "r0hip_worker_create: in_flight above 8");
    ensure_init();
    w = new r0hip_worker;
    WorkerImpl& m = w->impl;
    m.max_po2 = max_po2;
    m.k = in_flight ? in_flight : 2;
    m.verify = verify;
    if (h_noise_key) memcpy(m.key, h_noise_key, sizeof m.key);
    else os_random_key(m.key);
    const size_t n = size_t(1) << max_po2;
    m.sets = std::vector<WorkerSet>(m.k + 1);
    for (auto& s : m.sets) {
      s.glob = DevBuf(kGlobalWords);
      s.index = DevBuf(n + 1);
      s.cycles = DevBuf(n * kCycleWords);
      s.offsets = DevBuf(1);
      s.values = DevBuf(1);
      s.txns = DevBuf(kTxnWords);
      s.bigint = DevBuf(1);
      s.cap_inj = 1, s.cap_txn = 1, s.cap_big = 4;
      HIP_OK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    HIP_OK(hipDeviceSynchronize());  // allocations complete before other streams use them
    for (size_t s = 0; s < m.sets.size(); s++) m.free_q.put(long(s));
    for (size_t t = 0; t < m.k; t++) m.provers.emplace_back([&m] { m.run_prover(); });
    if (m.verify) m.verifier = std::thread([&m] { m.run_verifier(); });
    m.uploader = std::thread([&m] { m.run_uploader(); });
    *out = w;
  });
  if (err && w) {
    w->impl.shutdown();
    delete w;
  }
  if (err) {
    drain_after_error();
    release_thread_memory();
  }
  return err;
}

extern "C" const char* r0hip_worker_submit(r0hip_worker* w, r0hip_worker_job* job) {
  return guarded([&] {
    R0_REQUIRE(w && job, "r0hip_worker_submit: null argument");
    WorkerImpl& m = w->impl;
    R0_REQUIRE(job->kind == R0HIP_JOB_RV32IM_TRACE || job->kind == R0HIP_JOB_RECURSION ||
                   job->kind == R0HIP_JOB_RV32IM_BACKS || job->kind == R0HIP_JOB_RECURSION_PROGRAM ||
                   job->kind == R0HIP_JOB_RECURSION_INPUT,
               "r0hip_worker_submit: unknown job kind");
    BacksInfo info;
    R0_REQUIRE(job->suite >= 0 && job->suite <= 2, "r0hip_worker_submit: unknown hash suite");
    R0_REQUIRE(job->po2 <= m.max_po2, "r0hip_worker_submit: po2 " + std::to_string(job->po2) +
                                          " above the worker's max_po2 " + std::to_string(m.max_po2));
    R0_REQUIRE(!job->seal_cap || job->h_seal, "r0hip_worker_submit: h_seal is NULL with seal_cap > 0");
    if (job->kind == R0HIP_JOB_RECURSION) {
      const r0hip_recursion_input& in = job->recursion;
      R0_REQUIRE(job->po2 >= 11, "r0hip_worker_submit: recursion po2 below 11 (the ZK rows need po2 >= 11)");
      R0_REQUIRE(in.n_cycles <= (size_t(1) << job->po2) - 1024,
                 "r0hip_worker_submit: program longer than 2^po2 - ZK_CYCLES rows");
      R0_REQUIRE(in.h_ctrl && (in.h_wom || !in.n_wom) && (in.h_cycles || !in.n_cycles) && (in.h_iops || !in.n_iops) &&
                     (in.h_code_roots || !in.n_code_roots),
                 "r0hip_worker_submit: recursion job: null argument");
    } else if (job->kind == R0HIP_JOB_RECURSION_PROGRAM) {
      const r0hip_recursion_input& in = job->recursion;
      R0_REQUIRE(job_program(job), "r0hip_worker_submit: recursion program job: program is NULL");
      const RecursionProgramShape sh = recursion_program_shape(job_program(job));
      R0_REQUIRE(sh.suite == job->suite, "r0hip_worker_submit: the program's suite " + std::to_string(sh.suite) +
                                             " is not the job's suite " + std::to_string(job->suite));
      R0_REQUIRE(sh.po2 == job->po2, "r0hip_worker_submit: the program's po2 " + std::to_string(sh.po2) +
                                         " is not the job's po2 " + std::to_string(job->po2));
      R0_REQUIRE(in.n_cycles == sh.code_rows, "r0hip_worker_submit: n_cycles " + std::to_string(in.n_cycles) +
                                                  " is not the program's code_rows " + std::to_string(sh.code_rows));
      R0_REQUIRE((in.h_wom || !in.n_wom) && (in.h_cycles || !in.n_cycles) && (in.h_iops || !in.n_iops) &&
                     (in.h_code_roots || !in.n_code_roots),
                 "r0hip_worker_submit: recursion program job: null argument");
    } else if (job->kind == R0HIP_JOB_RECURSION_INPUT) {
      const auto* ij = reinterpret_cast<const r0hip_worker_input_job*>(job);
      R0_REQUIRE(ij->program, "r0hip_worker_submit: recursion input job: program is NULL");
      const RecursionProgramShape sh = recursion_program_shape(ij->program);
      R0_REQUIRE(sh.suite == job->suite, "r0hip_worker_submit: the program's suite " + std::to_string(sh.suite) +
                                             " is not the job's suite " + std::to_string(job->suite));
      R0_REQUIRE(sh.po2 == job->po2, "r0hip_worker_submit: the program's po2 " + std::to_string(sh.po2) +
                                         " is not the job's po2 " + std::to_string(job->po2));
      R0_REQUIRE((ij->h_input || !ij->n_input) && (ij->h_output || !ij->output_cap) &&
                     (job->recursion.h_code_roots || !job->recursion.n_code_roots),
                 "r0hip_worker_submit: recursion input job: null argument");
    } else if (job->kind == R0HIP_JOB_RV32IM_BACKS) {
      R0_REQUIRE(job->po2 >= 2, "r0hip_worker_submit: po2 out of range");
      check_backs_trace(job->trace, "r0hip_worker_submit");
      info = check_backs(job->backs, size_t(1) << job->po2, "r0hip_worker_submit");
    } else {
      const r0hip_trace_input& t = job->trace;
      R0_REQUIRE(job->po2 >= 2, "r0hip_worker_submit: po2 out of range");
      R0_REQUIRE(t.h_global && t.h_inj_index && t.preflight.cycles, "r0hip_worker_submit: trace job: null argument");
      R0_REQUIRE((t.preflight.txns_len == 0 || t.preflight.txns) &&
                     (t.preflight.bigint_bytes_len == 0 || t.preflight.bigint_bytes),
                 "r0hip_worker_submit: trace job: null trace array with a nonzero count");
      R0_REQUIRE(job->n_bigint == 0 || job->h_bigint, "r0hip_worker_submit: h_bigint is NULL with n_bigint > 0");
    }
    job->error = nullptr;
    job->seal_len = 0;
    job->verified = 0;
    job->verify_ms = 0;
    job->prove_ms = 0;
    {
      std::lock_guard<std::mutex> lk(m.mu);
      R0_REQUIRE(!m.stopping, "r0hip_worker_submit: the worker is shutting down");
      // the last thing that can refuse: a queued job holds the program until finish()
      if (job_holds_program(job)) recursion_program_acquire(job_program(job));
      job->ticket = m.next_ticket++;
      m.outstanding++;
      m.fifo.emplace_back(job, info);
      if (m.witness_check) m.checked_jobs.insert(job);
      // with a preflight pool a kind-4 job goes to its queue too, in the same (ticket) order
      if (job->kind == R0HIP_JOB_RECURSION_INPUT && m.pool.push(job)) m.pooled_jobs.insert(job);
    }
    m.cv_in.notify_one();
  });
}

extern "C" const char* r0hip_worker_set_witness_check(r0hip_worker* w, int on) {
  return guarded([&] {
    R0_REQUIRE(w, "r0hip_worker_set_witness_check: w is NULL");
    std::lock_guard<std::mutex> lk(w->impl.mu);
    w->impl.witness_check = on != 0;
  });
}

extern "C" const char* r0hip_worker_set_preflight_threads(r0hip_worker* w, uint32_t n, uint32_t* was) {
  return guarded([&] {
    R0_REQUIRE(w, "r0hip_worker_set_preflight_threads: w is NULL");
    R0_REQUIRE(n <= 8, "r0hip_worker_set_preflight_threads: n " + std::to_string(n) + " above 8");
    WorkerImpl& m = w->impl;
    // under mu to the end: no submit between the check and the new pool
    std::lock_guard<std::mutex> lk(m.mu);
    R0_REQUIRE(!m.stopping, "r0hip_worker_set_preflight_threads: the worker is shutting down");
    R0_REQUIRE(m.outstanding == 0, "r0hip_worker_set_preflight_threads: n " + std::to_string(n) + " refused with " +
                                       std::to_string(m.outstanding) + " jobs outstanding");
    // nothing outstanding: the pool's queue is empty and every slot is back, so its threads only wait
    const uint32_t now = m.pool.threads();
    if (n != now) m.pool.resize(n, uint32_t(m.k));
    if (was) *was = now;
  });
}

extern "C" const char* r0hip_worker_get_stats(r0hip_worker* w, r0hip_worker_stats* out, size_t out_size) {
  return guarded([&] {
    R0_REQUIRE(w, "r0hip_worker_get_stats: w is NULL");
    R0_REQUIRE(out, "r0hip_worker_get_stats: out is NULL");
    R0_REQUIRE(out_size == sizeof(r0hip_worker_stats), "r0hip_worker_get_stats: out_size " + std::to_string(out_size) +
                                                           " is not sizeof(r0hip_worker_stats) " +
                                                           std::to_string(sizeof(r0hip_worker_stats)));
    WorkerImpl& m = w->impl;
    r0hip_worker_stats st{};
    uint64_t bytes = 0;
    const PreflightPoolStats ps =
        m.pool.stats([&](const PfSlot& s) { bytes += s.bytes.load(std::memory_order_relaxed); });
    st.preflight_threads = ps.threads;
    st.preflight_slots = ps.slots;
    st.peak_slots_in_use = ps.peak_slots_in_use;
    st.pool_jobs = ps.jobs;
    st.slot_bytes = bytes;
    st.pool_busy_ms = ps.busy_ms;
    {
      std::lock_guard<std::mutex> lk(m.stats_mu);
      st.inline_jobs = m.inline_jobs;
      st.uploader_preflight_ms = m.uploader_preflight_ms;
      st.uploader_wait_preflight_ms = m.uploader_wait_preflight_ms;
    }
    *out = st;
  });
}

extern "C" const char* r0hip_worker_wait(r0hip_worker* w, r0hip_worker_job** done, int64_t timeout_ms) {
  return guarded([&] {
    R0_REQUIRE(w && done, "r0hip_worker_wait: null argument");
    *done = nullptr;
    WorkerImpl& m = w->impl;
    std::unique_lock<std::mutex> lk(m.mu);
    if (m.outstanding == 0) return;
    auto ready = [&] { return !m.finished.empty(); };
    if (timeout_ms < 0) m.cv_done.wait(lk, ready);
    else if (!m.cv_done.wait_for(lk, std::chrono::milliseconds(std::min<int64_t>(timeout_ms, int64_t(1) << 40)), ready))
      return;
    *done = m.finished.front();
    m.finished.pop_front();
    m.outstanding--;
  });
}

extern "C" const char* r0hip_worker_destroy(r0hip_worker* w) {
  const char* err = guarded([&] {
    R0_REQUIRE(w, "r0hip_worker_destroy: null argument");
    w->impl.shutdown();
    delete w;
  });
  // the sets are freed; the calling thread keeps no device memory
  drain_after_error();
  release_thread_memory();
  return err;
}
