// Host-side runtime shared by the C ABI (api.cpp), the segment prover
// (prover.cpp) and the kernel launchers: error plumbing, the per-process HIP
// stream, cached constant tables in HBM, and the launcher declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "bb31.h"

struct r0hip_bigint_back;  // include/r0hip.h
struct r0hip_recursion_program;
struct r0hip_opening;
struct r0hip_constraint_report;

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      throw std::runtime_error(std::string(#expr) + " failed: " + hipGetErrorString(e_) +     \
                               " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")");      \
  } while (0)

#define R0_REQUIRE(cond, msg)                                             \
  do {                                                                    \
    if (!(cond)) throw std::runtime_error(std::string("r0hip: ") + (msg)); \
  } while (0)

namespace r0 {

// Per-process stream on the current device (created by r0hip_init / lazily).
hipStream_t stream();
void ensure_init();
// One process-wide stream for copies that run beside every thread's work
// (r0hip_memcpy_d2h_start).
hipStream_t copy_stream();
// [p, p + bytes) lies inside one live r0hip_host_alloc block
bool host_pinned(const void* p, size_t bytes);

// Constant tables kept resident in HBM for the life of the process, keyed by a
// string; `gen` runs on the host once per key.
const uint32_t* dev_table(const std::string& key, const std::function<std::vector<uint32_t>()>& gen);

// Per-thread scratch slots. A slot is one buffer reused across calls in stream order (a
// later use on the thread's stream runs after every earlier kernel that read it); two
// buffers that are live at the same time need two slots. Every slot id is named here.
enum ScratchSlot : int {
  kSlotDefault = 0,
  // batch_evaluate_any (eltwise.hip)
  kSlotEvalPartial = 2,
  kSlotEvalPoly = 9,
  kSlotEvalBegin = 10,
  kSlotEvalIdx = 11,
  kSlotEvalTable = 12,
  // poly_divide_rows (eltwise.hip): row tables alternate between two slots per batch
  kSlotDivRows = 3,
  kSlotDivRowsAlt = 103,
  kSlotDivRem = 4,
  kSlotDivLaneV = 5,
  kSlotDivLaneM = 6,
  kSlotDivBlockV = 7,
  kSlotDivBlockM = 8,
  // eval_check (prover.cpp)
  kSlotEcPolyMix = 20,
  kSlotEcVinv = 21,
  kSlotEcAcc = 22,
  kSlotEcMatFp = 23,
  kSlotEcMatExt = 24,
  kSlotEcPolyMixNb = 25,
  kSlotEcColPtr = 26,
  kSlotEcInterp = 28,   // the interpreter's slot file (eval_interp.hip), a run-time circuit's only
  kSlotEcGatePtr = 29,  // the zero scan's column pointers and its two flag words
  kSlotEcGateFlags = 30,
  kSlotEcUniform = 27,  // prover uploads (prover.cpp): evaluation points per group (3 groups), check points,
  // mix_poly_coeffs row lists, combos deltas, query gather tables
  kSlotTapXs = 33,  // .. 35
  kSlotCheckXs = 37,
  kSlotMixWhich = 38,
  kSlotMixWhichCheck = 39,
  kSlotCombosDeltas = 44,
  kSlotQueryBases = 45,
  kSlotQueryIds = 46,
  kSlotQueryOffs = 47,
  // mix_poly_coeffs (eltwise.hip)
  kSlotMixRows = 40,
  kSlotMixPows = 41,
  kSlotMixSeg = 42,
  kSlotMixSegCombo = 43,
  // per-op ABI (api.cpp)
  kSlotApiMixWhich = 50,
  kSlotApiDeltas = 51,
  kSlotApiRem = 52,
  kSlotApiRems = 53,
  kSlotApiGather = 54,
  kSlotApiPaths = 55,
  kSlotApiPathIdx = 56,
  // accumulation (recursion_accum.hip, accum.hip, bigint.cpp)
  kSlotRecAccVals = 60,
  kSlotRecAccProds = 61,
  kSlotAccTileSums = 62,
  kSlotBigIntRows = 63,
  kSlotBigIntStates = 64,
  // BigInt accumulator scans (bigint.cpp, bigint_accum.hip): the uploaded records, each
  // record's byte polynomial, the tile sums, the failing-EqZero word
  kSlotBigIntBacks = 65,
  kSlotBigIntDelta = 66,
  kSlotBigIntTileSums = 67,
  kSlotBigIntFail = 68,
  // recursion witness generation (recursion_witgen.hip): the uploaded preflight trace, the
  // exec runs, each cycle's first IOP value, hipcub temporary storage
  kSlotWitgenWom = 70,
  kSlotWitgenIops = 71,
  kSlotWitgenRuns = 72,
  kSlotWitgenIopIdx = 73,
  kSlotWitgenTemp = 74,
  kSlotWitgenRunKey = 88,  // .. 91: run keys and indices, sorted
  kSlotWitgenRunTemp = 92,
  // rv32im witness generation (rv32im_witgen.hip): the uploaded preflight trace, the cycle
  // lists per instruction arm, the lookup tables and the error record
  kSlotRvwgCycles = 75,
  kSlotRvwgTxns = 76,
  kSlotRvwgBigint = 77,
  kSlotRvwgLists = 78,
  kSlotRvwgTables = 79,
  kSlotRvwgKeys = 83,
  kSlotRvwgSortTemp = 84,
  kSlotRvwgCompact = 85,
  kSlotRvwgSlotTable = 86,
  // r0hip_prove_segment_trace (api.cpp): the injector's index, offsets and values
  kSlotRvInjIndex = 80,
  kSlotRvInjOffsets = 81,
  kSlotRvInjValues = 82,
  kSlotRvInitErr = 87,
  // the injector as Back records (api.cpp): the records and their payload words
  kSlotRvBackRecs = 93,
  kSlotRvBackWords = 94,
  // the constraint-rows check (prover.cpp): the report words, the first bad row's gathered taps
  // and the gather's tables; its kernels' tables and scratch reuse the eval_check slots, which
  // nothing else holds while the check runs
  kSlotRowsReport = 95,
  kSlotRowsTaps = 96,
  kSlotRowsBases = 97,
  kSlotRowsIds = 98,
  kSlotRowsOffs = 99,
};

// Scratch buffer reused across calls (grown on demand; stream-ordered use only).
void* scratch(size_t bytes, int slot = kSlotDefault);
// After an error: wait for whatever this thread already queued on its stream (ignoring the
// status), so no buffer is reused or handed to another thread while kernels still use it.
// Only a thread that has a stream drains; it never creates one.
void drain_after_error() noexcept;
// At the end of every entry point, with this thread's stream drained: hand the thread's idle
// pool and scratch blocks to the shared lists, where any thread's next request finds them (as
// an exiting worker thread's are handed over). A caller's thread — one that proves and
// returns, or the calling thread of r0hip_prove_segments, which runs a prover itself — then
// keeps no device memory between calls.
void release_thread_memory() noexcept;

// Completion mode of the calling thread (r0hip_set_deferred; off on every new thread). While it
// is on, the C ABI's device-only entry points return with their work queued on the thread's
// stream, and the rules that rest on "every call drains" change as follows:
//   - the thread's pool and scratch blocks stay with the thread (its stream orders their reuse)
//     and go to the shared lists only at a return that drained: release_thread_memory does
//     nothing while work is queued;
//   - inside a call that will return queued, upload_async stages every source (the caller's
//     array may die before the copy runs); the arena is recycled at each drain, and a full
//     arena drains the stream and starts over instead of stacking a second one;
//   - a thread that exits with work queued leaks its blocks, stream and arena (~ThreadCtx can
//     make no HIP call), so a deferred thread synchronises before it exits.
// set_deferred_mode returns the previous mode; turning the mode off drains the stream first (an
// asynchronous error of the queued work is thrown, with the mode already off).
bool deferred_mode() noexcept;
bool set_deferred_mode(bool on);
// An entry point that will return with its work queued says so before it does any work; every
// entry point ends with the stream drained, or with work left queued (deferred mode).
void call_will_queue() noexcept;
void call_drained() noexcept;
void call_queued() noexcept;
void call_stats(uint64_t out[3]) noexcept;  // this thread's calls: all, drained, queued
// Make stream `other` wait for the work this thread has queued so far (an event on the thread's
// stream); nothing to do when the thread's last call drained.
void order_after_thread_work(hipStream_t other);

// One proof's independent work on several streams (r0hip_set_proof_streams; 1 on every new
// thread, which is the single-stream launch sequence with no extra HIP call). With n >= 2 a
// function may move independent work to one of the thread's side streams, created on first use
// and handed over or leaked with the main stream when the thread exits. Invariant: every
// function that forks has joined before it returns (the main stream waits for the side stream),
// so "main stream drained" still means "all of this thread's work is done", and
// release_thread_memory, download, the deferred-mode rules and order_after_thread_work hold
// unchanged. Buffers used on a side stream are requested before the fork and released after the
// join. After an error drain_after_error also waits for the side streams: an exception between
// a fork and its join hands no block back while side kernels run.
constexpr uint32_t kMaxProofStreams = 3;  // main + 2 side streams; with the copy stream, HIP's 4 queues
uint32_t proof_streams() noexcept;        // the thread's setting
void set_proof_streams(uint32_t n);       // 1..kMaxProofStreams, the caller has drained
// The setting in effect: 1 while kernel timing is on (KScope and Profile bracket work with events
// on the main stream, which must keep covering it).
uint32_t active_proof_streams() noexcept;
hipStream_t side_stream(int k);  // k = 1, 2
// `waiter` runs what is queued on it from now on after everything queued on `on` so far (one
// event record and one wait); fork(k) orders side stream k after the main stream, join(k) the
// main stream after side stream k.
void order_stream_after(hipStream_t waiter, hipStream_t on);
void fork(int k);
void join(int k);

// Stream-ordered host->device upload through a pinned bump arena, so the caller's
// host data may die immediately. The arena is recycled by stage_reset() (call only
// when the stream is idle). Exception: a source of 64 KiB or more inside a live
// r0hip_host_alloc block is copied to the device directly, with no staging, so it must
// stay valid until the copy has run (a call that returns queued never takes this path). Rule
// for every entry point that takes host arrays: drain this thread's stream (or stage_reset)
// before returning to the caller, or, for one that may return deferred, pass host data only
// through upload_async.
void upload_async(void* d_dst, const void* h_src, size_t bytes);
void stage_reset();
// `bytes` of the arena for a producer that writes its upload in place: page-locked, 256-byte
// aligned, the calling thread's until its next stage_reset; copy from it on the thread's stream.
void* stage_host(size_t bytes);
// Device-to-host copy in stream order, complete on return (this thread's stream is drained):
// small copies into pageable memory bounce through the page-locked arena.
void download(void* h_dst, const void* d_src, size_t bytes);
// The same host-to-device (small pageable sources bounce through the arena), complete on return.
void upload(void* d_dst, const void* h_src, size_t bytes);

// Optional kernel-level timing (HIP events on the library stream around each
// launcher), with the launcher's algorithmic HBM bytes and modmul-equivalent count
// (field multiplications of the restated algorithm) for roofline reporting.
struct KScope {
  KScope(const char* name, double alg_bytes, double alg_modmuls = 0);
  ~KScope();
  int idx = -1;
};
void ktimer_enable(bool on);
std::string ktimer_report();  // "name=total_ms:calls:alg_bytes:alg_modmuls;..." (synchronises)

// Device-memory accounting, the reference HAL's MemoryTracker (zkp/src/hal/mod.rs:292-317):
// `live` = bytes of the buffers handed out (pooled DevBufs and per-thread scratch), `reserved`
// = bytes held from hipMalloc (live + free pool blocks + constant tables), their peaks since
// the last reset, and the number of hipMalloc calls the library has made.
struct MemStats {
  uint64_t live, peak_live, reserved, peak_reserved, mallocs;
};
MemStats mem_stats();
void mem_reset_peak();

// A named host range for rocprofv3 --marker-trace (roctx), the reference's scope! spans
// (core/src/perf.rs:40-72; prover.rs, fri.rs, merkle.rs use the same names). Like the
// reference's, a range covers the host work of a phase: the device work it queues runs
// asynchronously on the thread's stream and shows up in the kernel trace.
struct Span {
  explicit Span(const char* name);
  ~Span();
  Span(const Span&) = delete;
  Span& operator=(const Span&) = delete;
};

// Witness groups that may still be uploading when a proof starts (the segment pipeline),
// copied in column chunks of chunk_cols(g): wait(g, col_end, s) returns once columns
// [0, col_end) of group g (0 code, 1 data, 2 accum, 3 global) have their copies queued,
// with stream s made to wait for those copies on the device.
struct UploadGate {
  virtual void wait(int group, size_t col_end, hipStream_t s) const = 0;
  virtual size_t chunk_cols(int group) const = 0;
 protected:
  ~UploadGate() = default;
};

// Workgroups for a 1-D launch of a lanes at b per workgroup. An AQL dispatch counts
// work-items in 32 bits, so a grid of 2^32 or more lanes cannot launch; such sizes go
// through grid_stride() instead.
inline unsigned div_up(size_t a, size_t b) {
  const size_t g = (a + b - 1) / b;
  R0_REQUIRE(g * b < (size_t(1) << 32), "1-D launch of " + std::to_string(a) + " lanes exceeds the 32-bit grid");
  return unsigned(g);
}
// Grid for element-wise kernels that stride over n elements (for (i = gid; i < n; i += lanes)):
// at most 2^20 workgroups (every CU stays busy), never above the 32-bit grid.
inline unsigned grid_stride(size_t n, size_t b) {
  const size_t g = (n + b - 1) / b;
  return unsigned(g < (size_t(1) << 20) ? g : (size_t(1) << 20));
}

// ---- launchers (all asynchronous on `s`) -----------------------------------
// NTT family (ntt.hip). Sizes are log2 of the per-polynomial length.
void ntt_evaluate(hipStream_t s, uint32_t* out, const uint32_t* in, size_t count, uint32_t log_out,
                  uint32_t expand_bits);
void ntt_interpolate(hipStream_t s, uint32_t* io, size_t count, uint32_t log_n, bool zk_shift);
void ntt_interpolate_from(hipStream_t s, uint32_t* io, const uint32_t* src, size_t count, uint32_t log_n,
                          bool zk_shift);
void bit_reverse(hipStream_t s, uint32_t* io, size_t count, uint32_t log_n);
// the same permutation on rows of 2^log_n FpExt elements (AoS, 4 words each)
void bit_reverse_ext(hipStream_t s, uint32_t* io, size_t count, uint32_t log_n);
void zk_shift(hipStream_t s, uint32_t* io, size_t count, uint32_t log_n);

// Hashes (hash.hip). suite: 0 = poseidon2, 1 = sha-256, 2 = poseidon254.
void hash_rows(hipStream_t s, int suite, uint32_t* out, const uint32_t* matrix, size_t rows, size_t cols);
// Row hashes over a matrix that arrives in column ranges: `cols` columns starting at
// `chunk` (column-major, `rows` per column), continuing the per-row sponge held in `state`
// (8 words per row) unless `first`; the `last` range writes the digests to `out`. Every
// range but the last must hold a multiple of 16 columns. Poseidon2 and SHA-256 only.
void hash_rows_range(hipStream_t s, int suite, uint32_t* out, uint32_t* state, const uint32_t* chunk, size_t rows,
                     size_t cols, bool first, bool last);
void hash_fold(hipStream_t s, int suite, uint32_t* io, size_t input_size, size_t output_size);
// Full merkle tree: nodes[rows..2rows) = leaves, hashes every layer up to the root.
void merkle_tree(hipStream_t s, int suite, uint32_t* nodes, const uint32_t* matrix, size_t rows, size_t cols);
// The layers above leaves already in nodes[rows..2rows). `cols` (the matrix's column count,
// SIZE_MAX if unknown) lets Poseidon2 and SHA-256 layers skip zero subtrees (hash.hip, ZeroSub).
void merkle_layers(hipStream_t s, int suite, uint32_t* nodes, size_t rows, size_t cols = SIZE_MAX);
// A seal's Merkle openings up to the comparison with the tree (MerkleVerifier::check, verify_core.h):
// per opening, hash_elems of the row at words[row_off .. + cols), then `levels` pair hashes with the
// path digests at words[path_off ..], sides from the heap index. Suites 0 and 1. The launcher
// checks the host copy of the table (merkle_open_check: cols in [1, 256], levels <= 40, every range
// inside n_words; throws before any device call), uploads it to d_open and queues one kernel on s:
// d_out gets 8 digest words per opening, then one status word per opening (0 computed, 2 a
// Poseidon2 path digest word >= p). Poseidon2 row words must be canonical (< p). Suite 2
// (Poseidon254, one opening per lane: the row hash as p254_rows_kernel has it, Montgomery words
// decoded first as hash_elems(2, ...) decodes them, the path on p254_hash_pair) is taken only with
// allow_p254, which the caller sets from verify_device_poseidon254() once per check, so a switch
// flipped by another thread in mid-check changes nothing of that check. Its row words must be
// canonical too, its path digests are any 256-bit words (p254_from_digest reduces them, as on the
// host) and its status is always 0.
constexpr uint32_t kMerkleOpenMaxCols = 256, kMerkleOpenMaxLevels = 40;
// r0hip_set_verify_device_poseidon254: process-wide, off by default, read at each check (verify.cpp).
bool verify_device_poseidon254();
void merkle_open_check(int suite, size_t n_words, const r0hip_opening* h_open, size_t n_open, bool allow_p254 = false);
void merkle_open(hipStream_t s, int suite, const uint32_t* d_words, size_t n_words, const r0hip_opening* h_open,
                 size_t n_open, r0hip_opening* d_open, uint32_t* d_out, bool allow_p254 = false);
// Host arrays in and out on the calling thread's stream, complete on return: the words go up
// once through the thread's staging arena, the table and the outputs come from its pool.
void merkle_open_host(int suite, const uint32_t* h_words, size_t n_words, const r0hip_opening* h_open, size_t n_open,
                      uint32_t* h_digests, uint32_t* h_status, bool allow_p254 = false);

// The constraint-rows check (prover.cpp; r0hip_constraint_rows): the circuit's constraint
// polynomial on the 2^po2 rows of the witness groups as they are (accum, code, data: device
// matrices, column-major), with poly_mix given. vals: where the per-row values go (2^po2 FpExt,
// AoS), or null for thread scratch. The report names the bad rows; when there are any, the first
// one's taps are gathered to the host and constraint_term (verify.cpp) names the term, from host
// copies of mix and global (read back when null). Drains the thread's stream.
struct CircuitDef;
void constraint_rows_run(const CircuitDef& c, size_t po2, const uint32_t* const* groups, const uint32_t* mix,
                         const uint32_t* global, const uint32_t* h_mix, const uint32_t* h_global, FpExt poly_mix,
                         uint32_t* vals, r0hip_constraint_report* report);
int32_t constraint_term(const CircuitDef& c, const uint32_t* taps, const uint32_t* mix, const uint32_t* global,
                        FpExt poly_mix);
// r0hip_set_witness_check: the calling thread's mode (off on every new thread). While it is on,
// prove_segment runs constraint_rows_run on its three groups in their final form, before the
// accum group is committed, and throws "constraint check failed: ..." instead of proving a
// witness that violates a constraint.
bool witness_check_mode() noexcept;
bool set_witness_check_mode(bool on) noexcept;  // returns the previous mode
// rows_report (eltwise.hip): over n FpExt values, out[0..1] = how many are nonzero (64 bits),
// out[2] = the smallest nonzero index, out[3..19) = the 16 smallest in ascending order
// (0xFFFFFFFF where there is none); 19 words.
void rows_report(hipStream_t s, const uint32_t* vals, size_t n, uint32_t* out);
// zero_scan (eltwise.hip): cols is a device table of n <= 64 pointers to `words` words each;
// flags (two device words, cleared here first) gets bit g set when column g holds a nonzero word.
void zero_scan(hipStream_t s, const uint32_t* const* cols, int n, size_t words, uint32_t* flags);
// The scan over device columns given on the host, its flags read back (prover.cpp): bit g of the
// result = column g is zero in all `words` words. Drains the thread's stream.
uint64_t zero_scan_mask(const std::vector<const uint32_t*>& cols, size_t words);
// The kernels the calling thread's last eval_check launched and the kernels its program has (the
// zero scan's effect, prover.cpp; r0hip_eval_check_launched). 0, 0 before the first call and after
// an interpreted one.
void eval_check_launched(int out[2]) noexcept;

// Element-wise and polynomial kernels (eltwise.hip).
void eltwise_add(hipStream_t s, uint32_t* out, const uint32_t* a, const uint32_t* b, size_t n);
void eltwise_copy(hipStream_t s, uint32_t* out, const uint32_t* in, size_t n);
void eltwise_zeroize(hipStream_t s, uint32_t* io, size_t n);
void fill_uniform(hipStream_t s, uint32_t* out, size_t n, uint64_t seed);
// A ChaCha20 key and nonce as the RFC 8439 state words (little-endian), passed to the kernel by
// value. fill_chacha20: out[i] = keystream words 4i..4i+3 (block counter from 0) as a 128-bit
// little-endian integer mod p, n <= 2^34.
struct ChaChaKey {
  uint32_t key[8];
  uint32_t nonce[3];
};
void fill_chacha20(hipStream_t s, uint32_t* out, size_t n, const ChaChaKey& key);
// 32 bytes from getrandom(2); throws when the OS gives none (there is no weaker source)
void os_random_key(uint32_t key[8]);
// The ZK noise of a recursion proof (api.cpp): fill `count` words of noise matrix `which` (0 the
// data group's, 1 the accum group's) on stream s. keyed_noise: the ChaCha20 stream under `key`
// (8 words, read at each fill) with nonce {which, lo32(stream_id), hi32(stream_id)}.
using RecursionNoise = std::function<void(hipStream_t s, uint32_t* out, size_t count, uint32_t which)>;
RecursionNoise keyed_noise(const uint32_t* key, uint64_t stream_id);
// ctrl_cached (devmem.h): the control group's commitment, made earlier from d_ctrl and kept
struct CachedGroup;
std::vector<uint32_t> prove_recursion(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom,
                                      size_t n_wom, const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                      size_t n_iops, const RecursionNoise& noise_fill, std::vector<uint32_t>* mix,
                                      const CachedGroup* ctrl_cached = nullptr);
// A recursion program handle (r0hip_recursion_program, api.cpp) for the worker: its shape, a use
// count taken per proof or queued job (destroy refuses while one is held), and the proof of
// r0hip_prove_recursion_program on the calling thread's stream.
struct RecursionProgramShape {
  int suite;
  uint32_t po2;
  size_t code_rows;
  const uint32_t* control_id;  // 8 words
};
RecursionProgramShape recursion_program_shape(const r0hip_recursion_program* h);
void recursion_program_acquire(const r0hip_recursion_program* h);
void recursion_program_release(const r0hip_recursion_program* h) noexcept;
std::vector<uint32_t> prove_recursion_program(const r0hip_recursion_program* h, const uint32_t* h_wom, size_t n_wom,
                                              const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                              size_t n_iops, const RecursionNoise& noise_fill,
                                              std::vector<uint32_t>* mix);
// What recursion witness generation derives from the program alone (recursion_witgen.hip), kept
// on the device in one dedicated allocation: the exec runs, each cycle's first IOP value, the
// runs ordered by bucket, and on the host the runs per bucket.
struct RecursionWitgenPlan {
  uint32_t* buf = nullptr;
  size_t bytes = 0;
  const uint32_t *run_start = nullptr, *iop_idx = nullptr, *order = nullptr;
  uint32_t nruns = 0;
  size_t ncycles = 0;
  uint32_t counts[9] = {};
};
// h_cycles: {iop_idx, is_par_safe} per cycle. Runs today's run keys and their sort once on s and
// returns with s drained; recursion_witgen_plan_free gives the allocation back.
void recursion_witgen_plan(hipStream_t s, const uint32_t* ctrl, size_t total_cycles, const uint32_t* h_cycles,
                           size_t ncycles, RecursionWitgenPlan* plan);
void recursion_witgen_plan_free(RecursionWitgenPlan* plan) noexcept;
// recursion_witgen with the runs, their order and the bucket counts read from the plan: no run
// keys, no run sort and no host synchronisation before the final error read. pinned: h_wom and
// h_iops are page-locked and stay valid until s has drained (copied without staging).
void recursion_witgen_planned(hipStream_t s, const uint32_t* ctrl, uint32_t* data, uint32_t* global,
                              size_t total_cycles, const RecursionWitgenPlan& plan, const uint32_t* h_wom,
                              size_t n_wom, const uint32_t* h_iops, size_t n_iops, bool pinned);
// Proofs from a handle and the reference's `input` (api.cpp). prepare: the handle's op table and
// device plan, made once (thread-safe). preflight_into runs the handle's preflight; wom and iops
// may be page-locked. prove_recursion_program_input: preflight (into the thread's staging arena
// when h_wom is NULL, else the given page-locked arrays are taken as a finished preflight),
// planned witness generation, then prove_recursion_program's sequence.
struct RecursionInputCounts {
  size_t n_wom, n_iops, n_output;
};
RecursionInputCounts recursion_program_prepare_input(const r0hip_recursion_program* h);
// the same counts when the plan exists already, without touching the device (any thread); false:
// the handle has no plan yet and only recursion_program_prepare_input can make it
bool recursion_program_planned_counts(const r0hip_recursion_program* h, RecursionInputCounts* out);
void recursion_program_preflight_into(const r0hip_recursion_program* h, const uint32_t* h_input, size_t n_input,
                                      uint32_t* wom, uint32_t* iops, uint32_t* output);
std::vector<uint32_t> prove_recursion_program_input(const r0hip_recursion_program* h, const uint32_t* h_input,
                                                    size_t n_input, const uint32_t* h_wom, const uint32_t* h_iops,
                                                    uint32_t* output, const RecursionNoise& noise_fill,
                                                    std::vector<uint32_t>* mix);
// Program.code (rows x 23 words, row-major, on the device) into the control group: 23 columns
// of 2^po2 words, rows from n_words / 23 on zero, every word of the group written by this launch.
// form 0: each word x becomes Elem::from(x) (the Montgomery word of x mod p); form 1: copied.
void recursion_program_expand(hipStream_t s, uint32_t* ctrl, const uint32_t* code, size_t n_words, uint32_t po2,
                              int form);
void rv32im_accum_finalize(hipStream_t s, uint32_t* accum, size_t rows, size_t cols, size_t split, size_t last);
void rv32im_accum(hipStream_t s, const uint32_t* data, uint32_t* accum, const uint32_t* global,
                  const uint32_t* mix, size_t rows, size_t cols, size_t last);
// The accumulation a segment prover runs between the mix draw and the accum commit
// (rv32im prove/witgen/mod.rs:178-221, recursion prove/witgen.rs:138-177): `accum` holds the
// group as the witness generator left it (INVALID words, plus the recursion ZK noise rows);
// the circuit's accumulation fills it for `work_cycles` cycles, then INVALID words become 0.
struct AccumStep {
  uint32_t* accum;
  size_t work_cycles;
  bool fill_invalid = false;  // the buffer is reused: fill it with INVALID words first
  // rv32im: the trace's Back::BigInt records, whose accumulator states are injected with the
  // final mix before the step (witgen/mod.rs:178-205)
  const r0hip_bigint_back* bigint = nullptr;
  size_t n_bigint = 0;
  // the group starts as rv32im_prover_groups_init leaves it (0 where the reference's INVALID
  // would be zeroized, INVALID where phase 3 adds to it), with every row stepped: the zeroize
  // after the accumulation would change nothing and is skipped
  bool zeroed = false;
};
// BigIntAccum::step over the records (byte_poly.rs:403-470): 12 words per record (poly, term,
// total), in record order; throws on an invalid EqZero as the reference does
std::vector<uint32_t> rv32im_bigint_accum_states(const uint32_t* mix, const r0hip_bigint_back* backs, size_t n,
                                                 size_t rows);
// The same states computed on the device into d_states (n x 12 words), complete on return, with
// the host function's errors. Returns the records as uploaded (this thread's kSlotBigIntBacks).
const r0hip_bigint_back* rv32im_bigint_accum_states_device(hipStream_t s, uint32_t* d_states, const uint32_t* mix,
                                                           const r0hip_bigint_back* backs, size_t n, size_t rows);
// the scans themselves (bigint_accum.hip) over n <= 2^26 records in device memory, every
// poly_op in range; mix is on the host. *d_fail becomes the smallest index of a record whose
// EqZero goal is nonzero, 0xFFFFFFFF if there is none.
void bigint_accum_scan(hipStream_t s, uint32_t* d_states, const r0hip_bigint_back* d_backs, size_t n,
                       const uint32_t* mix, uint32_t* d_fail);
// the states scattered into accum columns 0..11 of each record's row (witgen/mod.rs:187-205)
void rv32im_bigint_inject(hipStream_t s, uint32_t* accum, size_t rows, const uint32_t* mix,
                          const r0hip_bigint_back* backs, size_t n);
// record k's row is d_rows[k * row_stride] (1: a row list; 7: the records themselves)
void bigint_scatter(hipStream_t s, uint32_t* accum, size_t rows, const uint32_t* d_rows, const uint32_t* d_states,
                    size_t n, size_t row_stride = 1);
// recursion circuit accumulation (recursion_accum.hip): compute, prefix product, verify
void recursion_accum(hipStream_t s, const uint32_t* ctrl, const uint32_t* global, const uint32_t* data,
                     const uint32_t* mix, uint32_t* accum, size_t steps, size_t cycles);
// recursion circuit witness generation (recursion_witgen.hip; risc0_circuit_recursion_cpu_witgen,
// recursion-sys/kernels/cxx/ffi.cpp:191-205): data (INVALID-filled) and global written from the
// control group and the preflight trace (WOM and IOP values 4 words each, cycles {iopIdx,
// isParSafe}); synchronises, throws on a failed check
void recursion_witgen(hipStream_t s, const uint32_t* ctrl, uint32_t* data, uint32_t* global, size_t total_cycles,
                      const uint32_t* h_wom, size_t n_wom, const uint32_t* h_cycles, size_t ncycles,
                      const uint32_t* h_iops, size_t n_iops);
void eltwise_sum_extelem(hipStream_t s, uint32_t* out, const uint32_t* in, size_t count, size_t to_add);
void fri_fold(hipStream_t s, uint32_t* out, const uint32_t* in, FpExt mix, size_t count);
void gather_sample(hipStream_t s, uint32_t* dst, const uint32_t* src, size_t idx, size_t size, size_t stride);
// Merkle openings' sibling paths (prove/merkle.rs:131-138) out of a node heap of heap_digests
// digests, root at 1: dst[(i*levels + k)*8 ..] = nodes[j] for k = 0, nodes[(j >> k) ^ 1] for
// k >= 1, j = idx[i] (device array), or j = one for every i when idx is null. The caller has
// checked every j; a node outside the heap is written as zeros, never read.
void merkle_paths(hipStream_t s, uint32_t* dst, const uint32_t* nodes, size_t heap_digests, const uint64_t* idx,
                  uint64_t one, size_t n, size_t levels);
void mix_poly_coeffs(hipStream_t s, uint32_t* out, const uint32_t* in, const uint32_t* combos_dev,
                     const std::vector<uint32_t>& combos_host, FpExt mix_start, FpExt mix,
                     size_t input_size, size_t count);
void batch_evaluate_any(hipStream_t s, const uint32_t* coeffs, size_t poly_count, uint32_t log_n,
                        const uint32_t* which, const uint32_t* xs, uint32_t* out, size_t eval_count);
// the same with `which` on the host (groups evaluations by polynomial without a D2H)
// bitrev: the coefficient rows are stored in bit-reversed order (row[j] = coefficient
// rev_{log_n}(j), as the inverse NTT leaves them); needs log_n >= kEvalBitrevMinLog
void batch_evaluate_any_host(hipStream_t s, const uint32_t* coeffs, size_t poly_count, uint32_t log_n,
                             const std::vector<uint32_t>& which, const uint32_t* xs, uint32_t* out,
                             bool bitrev = false);
constexpr uint32_t kEvalBitrevMinLog = 12;
void scatter(hipStream_t s, uint32_t* into, const uint32_t* index, const uint32_t* offsets,
             const uint32_t* values, size_t cycles, uint64_t limit = ~uint64_t(0));
void copy_elem_slice(hipStream_t s, uint32_t* into, const uint32_t* from, size_t rows, size_t cols,
                     size_t from_offset, size_t from_stride, size_t into_offset, size_t into_stride);
void prefix_products(hipStream_t s, uint32_t* io, size_t n);
// In-place synthetic division of `nrows` FpExt polys of length n (row r at io + r*n*4)
// by (x - z_k) for each of its z's, in order. zs/zbegin: flattened per-row lists.
// The remainders (must be zero) are written to rem_dev[row*maxz + k].
void poly_divide_rows(hipStream_t s, uint32_t* io, size_t n, const std::vector<std::vector<FpExt>>& zs,
                      uint32_t* rem_dev);

}  // namespace r0
