// C ABI (include/r0hip.h): the symbols a Rust `HipHal` binds in place of the
// reference's risc0_zkp_cuda_* / sppark_* / cust calls. Each entry point runs its
// kernels on the calling thread's stream and returns only when they have finished
// (risc0/sys/kernels/zkp/cuda/cuda.h:77-100 semantics), unless the thread has asked for
// deferred completion (r0hip_set_deferred): then the device-only entry points (wrap_dev)
// return with their work queued, as the stream-ordered CUDA HAL's do, and the entry points
// that hand data or a verdict to the host (wrap) drain first. Errors come back as a
// malloc'd string (risc0/sys/src/lib.rs:53-75 convention).
#include "../../include/r0hip.h"

#include <sys/random.h>

#include <cerrno>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "backs.h"
#include "circuit.h"
#include "devmem.h"
#include "eval_interp.h"
#include "plugin.h"
#include "recursion_preflight.h"
#include "runtime.h"
#include "rv32im_witgen.h"

namespace r0 {
void combos_sub(hipStream_t s, uint32_t* combos, const uint32_t* deltas, size_t rows, size_t width,
                size_t cycles);
void run_eval_check(const CircuitDef& c, uint32_t* check, const uint32_t* const* groups, const uint32_t* mix,
                    const uint32_t* global, FpExt poly_mix, size_t po2, const uint32_t* h_mix = nullptr,
                    const uint32_t* h_global = nullptr);
std::vector<uint32_t> prove_segment(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                    const uint32_t* data, const uint32_t* accum, uint32_t* global,
                                    bool write_version, uint32_t version, std::vector<uint32_t>* mix_out,
                                    const UploadGate* uploads = nullptr, const AccumStep* acc = nullptr,
                                    GroupWork* code_early = nullptr, const CachedGroup* code_cached = nullptr);
std::vector<uint32_t> prove_segment_cb(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                       const uint32_t* data, uint32_t* global, bool write_version, uint32_t version,
                                       std::vector<uint32_t>* mix_out, const AccumCallback& cb);
GroupWork commit_group_side(int k, int suite, const uint32_t* witness, size_t cols, size_t po2);
std::vector<uint32_t> commit_group_keep(hipStream_t s, int suite, uint32_t* coeffs, uint32_t* evaluated, uint32_t* nodes,
                                        const uint32_t* witness, size_t cols, size_t po2);
std::string last_profile();
FpExt constraint_rows_poly_mix(const uint32_t* h_poly_mix);  // the caller's four words, or the OS's
}  // namespace r0

using namespace r0;

namespace {
// The call's work is complete on return, and the calling thread's idle device memory goes back
// to the shared pool (release_thread_memory), so a caller's thread holds none between calls.
// `may_defer`: a device-only entry point (wrap_dev below). In the calling thread's deferred mode
// (r0hip_set_deferred) it returns with its work queued: no drain, and the thread keeps its
// memory, which queued work may still use. A failed call drains in either mode.
template <typename F>
const char* wrap(F f, bool may_defer = false) {
  const bool queue = may_defer && deferred_mode();
  try {
    if (queue) call_will_queue();
    f();
    if (queue) {
      call_queued();
      return nullptr;
    }
    HIP_OK(hipStreamSynchronize(stream()));
  } catch (const std::exception& e) {
    drain_after_error();
    call_drained();
    release_thread_memory();
    return strdup(e.what());
  } catch (...) {
    drain_after_error();
    call_drained();
    release_thread_memory();
    return strdup("r0hip: unknown error");
  }
  call_drained();
  release_thread_memory();
  return nullptr;
}
// Device-only entry points: device pointers and by-value scalars in, nothing handed to the host.
// Host arrays they take are consumed before they return (copied, or staged by upload_async).
template <typename F>
const char* wrap_dev(F f) {
  return wrap(f, true);
}
// host-only entry points: no stream, no device
template <typename F>
const char* wrap_nosync(F f) {
  try {
    f();
  } catch (const std::exception& e) {
    return strdup(e.what());
  }
  return nullptr;
}
uint32_t lg(size_t n, const char* what) {
  uint32_t r = 0;
  while ((size_t(1) << r) < n) r++;
  if ((size_t(1) << r) != n) throw std::runtime_error(std::string("r0hip: ") + what + " is not a power of two");
  return r;
}
FpExt fe(const uint32_t* w) { return FpExt{{w[0], w[1], w[2], w[3]}}; }
}  // namespace

extern "C" {

const char* r0hip_init(int device_ordinal) {
  return wrap([&] {
    set_device(device_ordinal);
    // warm the module (loads every code object once)
    (void)stream();
  });
}

const char* r0hip_device_info(char* name, size_t name_cap, uint64_t* total_mem) {
  return wrap([&] {
    ensure_init();
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIP_OK(hipGetDeviceProperties(&p, dev));
    if (name && name_cap) {
      strncpy(name, p.gcnArchName, name_cap - 1);
      name[name_cap - 1] = 0;
    }
    if (total_mem) *total_mem = p.totalGlobalMem;
  });
}

const char* r0hip_alloc(void** d_ptr, size_t bytes) {
  return wrap_dev([&] { *d_ptr = dev_alloc(bytes); });
}
const char* r0hip_free(void* d_ptr) {
  return wrap_dev([&] { dev_free(d_ptr); });
}
const char* r0hip_memset32(void* d_dst, uint32_t value, size_t count) {
  return wrap_dev([&] { HIP_OK(hipMemsetD32Async(d_dst, int(value), count, stream())); });
}
const char* r0hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
  return wrap([&] { upload(d_dst, h_src, bytes); });
}
const char* r0hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
  return wrap([&] { download(h_dst, d_src, bytes); });
}
const char* r0hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes) {
  return wrap_dev([&] { HIP_OK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, stream())); });
}
const char* r0hip_host_alloc(void** h_ptr, size_t bytes) {
  return wrap([&] { *h_ptr = host_alloc(bytes); });
}
const char* r0hip_host_free(void* h_ptr) {
  return wrap([&] { host_free(h_ptr); });
}
const char* r0hip_synchronize(void) {
  return wrap([] {});
}
const char* r0hip_set_deferred(int on, int* was) {
  return wrap_nosync([&] {
    if (was) *was = deferred_mode() ? 1 : 0;
    set_deferred_mode(on != 0);
  });
}
const char* r0hip_set_proof_streams(uint32_t n, uint32_t* was) {
  return wrap([&] {
    if (was) *was = proof_streams();
    set_proof_streams(n);
  });
}
const char* r0hip_set_witness_check(int on, int* was) {
  return wrap_nosync([&] {
    const bool w = set_witness_check_mode(on != 0);
    if (was) *was = w ? 1 : 0;
  });
}
const char* r0hip_testing_set_interp_chunk(uint32_t points, uint32_t* was) {
  return wrap_nosync([&] {
    const uint32_t w = set_interp_test_chunk(points);
    if (was) *was = w;
  });
}
const char* r0hip_testing_zero_scan(const uint32_t* d_matrix, size_t cols, size_t words, uint64_t* h_mask) {
  return wrap([&] {
    R0_REQUIRE(d_matrix && h_mask, "r0hip_testing_zero_scan: null argument");
    R0_REQUIRE(cols <= size_t(kMaxGates), "r0hip_testing_zero_scan: more than 64 columns");
    stage_reset();
    std::vector<const uint32_t*> ptrs(cols);
    for (size_t c = 0; c < cols; c++) ptrs[c] = d_matrix + c * words;
    *h_mask = zero_scan_mask(ptrs, words);
  });
}
const char* r0hip_eval_check_launched(int* out) {
  return wrap_nosync([&] {
    R0_REQUIRE(out != nullptr, "r0hip_eval_check_launched: null output");
    eval_check_launched(out);
  });
}
const char* r0hip_call_stats(uint64_t* out) {
  return wrap_nosync([&] {
    R0_REQUIRE(out != nullptr, "r0hip_call_stats: null output");
    call_stats(out);
  });
}

namespace {
struct PendingCopy {  // r0hip_memcpy_d2h_start's handle: the copy's completion on the copy stream
  hipEvent_t ev = nullptr;
  ~PendingCopy() {
    if (ev) (void)hipEventDestroy(ev);
  }
};
}  // namespace

const char* r0hip_memcpy_d2h_start(void* h_dst, const void* d_src, size_t bytes, void** h_copy) {
  return wrap_dev([&] {
    R0_REQUIRE(h_copy, "r0hip_memcpy_d2h_start: h_copy is NULL");
    *h_copy = nullptr;
    if (!bytes) return;
    R0_REQUIRE(h_dst && d_src, "r0hip_memcpy_d2h_start: null pointer");
    if (!host_pinned(h_dst, bytes)) {  // pageable: copied now, as r0hip_memcpy_d2h
      download(h_dst, d_src, bytes);
      return;
    }
    auto pc = std::make_unique<PendingCopy>();
    HIP_OK(hipEventCreateWithFlags(&pc->ev, hipEventDisableTiming));
    const hipStream_t cs = copy_stream();
    // after deferred calls the kernels that produce d_src may still be queued on this thread's
    // stream: the copy stream waits for them (nothing to wait for when the last call drained)
    order_after_thread_work(cs);
    HIP_OK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, cs));
    HIP_OK(hipEventRecord(pc->ev, cs));
    *h_copy = pc.release();
  });
}
const char* r0hip_copy_finish(void* h_copy, int block, int* done) {
  return wrap_nosync([&] {
    int fin = 1;
    if (h_copy) {
      auto* pc = static_cast<PendingCopy*>(h_copy);
      const hipError_t e = block ? hipEventSynchronize(pc->ev) : hipEventQuery(pc->ev);
      if (e == hipErrorNotReady) {
        fin = 0;
      } else {
        delete pc;  // the handle is spent either way
        HIP_OK(e);
      }
    }
    if (done) *done = fin;
  });
}
void r0hip_free_error(const char* err) { free(const_cast<char*>(err)); }

const char* r0hip_batch_expand_into_evaluate_ntt(uint32_t* d_out, const uint32_t* d_in, size_t count, uint32_t lg_out,
                                                 uint32_t expand_bits) {
  return wrap_dev([&] {
    R0_REQUIRE(lg_out >= expand_bits && lg_out <= 27, "bad NTT size");
    ntt_evaluate(stream(), d_out, d_in, count, lg_out, expand_bits);
  });
}
const char* r0hip_batch_interpolate_ntt(uint32_t* d_io, size_t count, uint32_t lg_size) {
  return wrap_dev([&] {
    R0_REQUIRE(lg_size <= 27, "bad NTT size");
    ntt_interpolate(stream(), d_io, count, lg_size, false);
  });
}
const char* r0hip_zk_shift(uint32_t* d_io, size_t count, uint32_t lg_size) {
  return wrap_dev([&] { zk_shift(stream(), d_io, count, lg_size); });
}
const char* r0hip_batch_bit_reverse(uint32_t* d_io, size_t count, uint32_t lg_size) {
  return wrap_dev([&] { bit_reverse(stream(), d_io, count, lg_size); });
}

const char* r0hip_batch_evaluate_any(uint32_t* d_out, const uint32_t* d_coeffs, size_t poly_count,
                                     uint32_t lg_poly_size, const uint32_t* d_which, const uint32_t* d_xs,
                                     size_t eval_count) {
  return wrap_dev([&] { batch_evaluate_any(stream(), d_coeffs, poly_count, lg_poly_size, d_which, d_xs, d_out, eval_count); });
}

const char* r0hip_mix_poly_coeffs(uint32_t* d_out, const uint32_t* d_in, const uint32_t* h_combos,
                                  const uint32_t* h_mix_start, const uint32_t* h_mix, size_t input_size,
                                  size_t count) {
  return wrap_dev([&] {
    std::vector<uint32_t> combos(h_combos, h_combos + input_size);
    uint32_t* d = static_cast<uint32_t*>(scratch(input_size * 4 + 16, kSlotApiMixWhich));
    upload_async(d, combos.data(), input_size * 4);
    mix_poly_coeffs(stream(), d_out, d_in, d, combos, fe(h_mix_start), fe(h_mix), input_size, count);
  });
}

const char* r0hip_fri_fold(uint32_t* d_out, const uint32_t* d_in, const uint32_t* h_mix, size_t count) {
  return wrap_dev([&] { fri_fold(stream(), d_out, d_in, fe(h_mix), count); });
}

const char* r0hip_combos_prepare(uint32_t* d_combos, const uint32_t* h_coeff_u, size_t combo_count, size_t cycles,
                                 const uint32_t* h_reg_sizes, const uint32_t* h_reg_combo_ids, size_t reg_count,
                                 const uint32_t* h_mix) {
  return wrap_dev([&] {
    size_t width = 1;
    for (size_t r = 0; r < reg_count; r++) width = std::max<size_t>(width, h_reg_sizes[r]);
    std::vector<FpExt> deltas((combo_count + 1) * width, fe_zero());
    FpExt cur = fe_one(), mix = fe(h_mix);
    size_t pos = 0;
    for (size_t r = 0; r < reg_count; r++) {
      for (size_t i = 0; i < h_reg_sizes[r]; i++) {
        FpExt& d = deltas[h_reg_combo_ids[r] * width + i];
        d = fe_add(d, fe_mul(cur, fe(h_coeff_u + 4 * (pos + i))));
      }
      cur = fe_mul(cur, mix);
      pos += h_reg_sizes[r];
    }
    for (size_t i = 0; i < 16; i++) {
      FpExt& d = deltas[combo_count * width];
      d = fe_add(d, fe_mul(cur, fe(h_coeff_u + 4 * pos)));
      pos++;
      cur = fe_mul(cur, mix);
    }
    uint32_t* dd = static_cast<uint32_t*>(scratch(deltas.size() * 16, kSlotApiDeltas));
    upload_async(dd, deltas.data(), deltas.size() * 16);
    combos_sub(stream(), d_combos, dd, combo_count + 1, width, cycles);
  });
}

const char* r0hip_poly_divide(uint32_t* d_poly, size_t size, uint32_t* h_remainder, const uint32_t* h_z) {
  return wrap([&] {
    std::vector<std::vector<FpExt>> zs{{fe(h_z)}};
    uint32_t* rem = static_cast<uint32_t*>(scratch(16, kSlotApiRem));
    poly_divide_rows(stream(), d_poly, size, zs, rem);
    HIP_OK(hipMemcpyAsync(h_remainder, rem, 16, hipMemcpyDeviceToHost, stream()));
  });
}

const char* r0hip_combos_divide(uint32_t* d_combos, size_t nchunks, const uint32_t* h_pows, const uint32_t* h_begin,
                                size_t cycles, int64_t* bad_chunk) {
  return wrap([&] {
    std::vector<std::vector<FpExt>> zs(nchunks);
    size_t maxz = 0;
    for (size_t i = 0; i < nchunks; i++) {
      for (uint32_t k = h_begin[i]; k < h_begin[i + 1]; k++) zs[i].push_back(fe(h_pows + 4 * k));
      maxz = std::max(maxz, zs[i].size());
    }
    std::vector<uint32_t> h(nchunks * std::max<size_t>(maxz, 1) * 4, 0);
    uint32_t* rem = static_cast<uint32_t*>(scratch(h.size() * 4 + 16, kSlotApiRems));
    HIP_OK(hipMemsetAsync(rem, 0, h.size() * 4, stream()));
    poly_divide_rows(stream(), d_combos, cycles, zs, rem);
    HIP_OK(hipMemcpyAsync(h.data(), rem, h.size() * 4, hipMemcpyDeviceToHost, stream()));
    HIP_OK(hipStreamSynchronize(stream()));
    *bad_chunk = -1;
    for (size_t i = 0; i < h.size(); i++)
      if (h[i]) {
        *bad_chunk = int64_t(i / (std::max<size_t>(maxz, 1) * 4));
        break;
      }
  });
}

const char* r0hip_eltwise_add_elem(uint32_t* d_out, const uint32_t* d_a, const uint32_t* d_b, size_t count) {
  return wrap_dev([&] { eltwise_add(stream(), d_out, d_a, d_b, count); });
}
const char* r0hip_eltwise_copy_elem(uint32_t* d_out, const uint32_t* d_in, size_t count) {
  return wrap_dev([&] { eltwise_copy(stream(), d_out, d_in, count); });
}
const char* r0hip_eltwise_zeroize_elem(uint32_t* d_io, size_t count) {
  return wrap_dev([&] { eltwise_zeroize(stream(), d_io, count); });
}
const char* r0hip_eltwise_sum_extelem(uint32_t* d_out, const uint32_t* d_in, size_t to_add, size_t count) {
  return wrap_dev([&] { eltwise_sum_extelem(stream(), d_out, d_in, count, to_add); });
}
const char* r0hip_eltwise_copy_elem_slice(uint32_t* d_into, const uint32_t* d_from, size_t from_rows,
                                          size_t from_cols, size_t from_offset, size_t from_stride,
                                          size_t into_offset, size_t into_stride) {
  return wrap_dev([&] {
    copy_elem_slice(stream(), d_into, d_from, from_rows, from_cols, from_offset, from_stride, into_offset,
                    into_stride);
  });
}
const char* r0hip_gather_sample(uint32_t* d_dst, const uint32_t* d_src, size_t idx, size_t size, size_t stride) {
  return wrap_dev([&] { gather_sample(stream(), d_dst, d_src, idx, size, stride); });
}
const char* r0hip_gather_sample_host(uint32_t* h_dst, const uint32_t* d_src, size_t idx, size_t size,
                                     size_t stride) {
  return wrap([&] {
    if (!size) return;
    R0_REQUIRE(h_dst && d_src, "gather_sample_host: null pointer");
    uint32_t* d = static_cast<uint32_t*>(scratch(size * 4, kSlotApiGather));
    gather_sample(stream(), d, d_src, idx, size, stride);
    download(h_dst, d, size * 4);
  });
}
const char* r0hip_merkle_paths_host(uint32_t* h_dst, const uint32_t* d_nodes, size_t heap_digests,
                                    const uint64_t* h_idx, size_t n, size_t levels) {
  return wrap([&] {
    if (!n) return;
    R0_REQUIRE(levels >= 1 && levels < 64, "merkle_paths_host: levels = " + std::to_string(levels) +
                                               " (an opening has the node itself and at most 62 siblings)");
    R0_REQUIRE(h_dst && d_nodes && h_idx, "merkle_paths_host: null pointer");
    // every index before any device work: the node and each sibling up to level levels-1 exist
    for (size_t i = 0; i < n; i++) {
      const uint64_t j = h_idx[i];
      auto at = [&] { return "merkle_paths_host: index " + std::to_string(j) + " (h_idx[" + std::to_string(i) + "])"; };
      R0_REQUIRE(j >= 1 && j < heap_digests, at() + " is outside [1, " + std::to_string(heap_digests) + ")");
      R0_REQUIRE(levels == 1 || (j >> (levels - 1)) >= 2,
                 at() + " has no sibling " + std::to_string(levels - 1) + " levels up (the root is node 1)");
    }
    const size_t words = n * levels * 8;
    uint32_t* d = static_cast<uint32_t*>(scratch(words * 4, kSlotApiPaths));
    const uint64_t* d_idx = nullptr;  // a single opening's index travels as a kernel argument
    if (n > 1) {
      uint64_t* di = static_cast<uint64_t*>(scratch(n * 8, kSlotApiPathIdx));
      upload_async(di, h_idx, n * 8);
      d_idx = di;
    }
    merkle_paths(stream(), d, d_nodes, heap_digests, d_idx, h_idx[0], n, levels);
    download(h_dst, d, words * 4);
  });
}
const char* r0hip_merkle_open_digests(int suite, const uint32_t* h_words, size_t n_words, const r0hip_opening* h_open,
                                      size_t n_open, uint32_t* h_digests, uint32_t* h_status) {
  return wrap([&] {
    // everything refused here and in merkle_open_check is refused before the first device call
    const bool p254 = suite == 2 && verify_device_poseidon254();  // the switch, read once for this call
    R0_REQUIRE(suite == 0 || suite == 1 || p254,
               "merkle_open_digests: suite = " + std::to_string(suite) + " has no device form (0 Poseidon2 or 1 SHA-256" +
                   (suite == 2 ? "; 2 Poseidon254 only after r0hip_set_verify_device_poseidon254(1))" : ")"));
    R0_REQUIRE(h_words || n_words == 0, "merkle_open_digests: h_words is NULL");
    R0_REQUIRE(h_open || n_open == 0, "merkle_open_digests: h_open is NULL");
    R0_REQUIRE(h_digests || n_open == 0, "merkle_open_digests: h_digests is NULL");
    R0_REQUIRE(h_status || n_open == 0, "merkle_open_digests: h_status is NULL");
    merkle_open_check(suite, n_words, h_open, n_open, p254);
    // the permutation's bounds (Poseidon2) and p254_pack8's column bound (Poseidon254) assume field
    // elements, as the verifier's read_elems guarantees
    if (suite == 0 || suite == 2)
      for (size_t i = 0; i < n_open; i++)
        for (uint32_t k = 0; k < h_open[i].cols; k++)
          R0_REQUIRE(h_words[h_open[i].row_off + k] < kP,
                     "merkle_open_digests: h_words[" + std::to_string(h_open[i].row_off + k) + "] (row of h_open[" +
                         std::to_string(i) + "]) is not a canonical field element");
    if (!n_open) return;
    merkle_open_host(suite, h_words, n_words, h_open, n_open, h_digests, h_status, p254);
  });
}
const char* r0hip_scatter(uint32_t* d_into, const uint32_t* d_index, const uint32_t* d_offsets,
                          const uint32_t* d_values, size_t cycles) {
  return wrap_dev([&] { scatter(stream(), d_into, d_index, d_offsets, d_values, cycles); });
}
const char* r0hip_prefix_products(uint32_t* d_io, size_t count) {
  return wrap_dev([&] { prefix_products(stream(), d_io, count); });
}
const char* r0hip_rv32im_accum_finalize(uint32_t* d_accum, size_t rows, size_t cols, size_t last_cycle) {
  // kUserAccumSplit = kLayout_TopAccum.columns[0].col (rv32im-sys/kernels/cxx/ffi.cpp:52,
  // layout.cpp.inc:6993-6999): the first machine accumulator column
  return wrap_dev([&] { rv32im_accum_finalize(stream(), d_accum, rows, cols, 23, last_cycle); });
}
const char* r0hip_rv32im_accum(const uint32_t* d_data, uint32_t* d_accum, const uint32_t* d_global,
                               const uint32_t* d_mix, size_t rows, size_t cols, size_t last_cycle) {
  return wrap_dev([&] { rv32im_accum(stream(), d_data, d_accum, d_global, d_mix, rows, cols, last_cycle); });
}
const char* r0hip_rv32im_bigint_accum_states(const uint32_t* h_mix, const r0hip_bigint_back* h_backs, size_t n,
                                             size_t rows, uint32_t* h_states) {
  return wrap_nosync([&] {
    R0_REQUIRE(h_mix && (n == 0 || (h_backs && h_states)), "r0hip_rv32im_bigint_accum_states: null argument");
    const std::vector<uint32_t> st = rv32im_bigint_accum_states(h_mix, h_backs, n, rows);
    if (n) memcpy(h_states, st.data(), st.size() * 4);
  });
}
const char* r0hip_rv32im_bigint_accum_states_device(uint32_t* d_states, const uint32_t* h_mix,
                                                    const r0hip_bigint_back* h_backs, size_t n, size_t rows) {
  return wrap([&] {
    if (n == 0) return;
    R0_REQUIRE(h_mix && h_backs && d_states, "r0hip_rv32im_bigint_accum_states_device: null argument");
    stage_reset();
    rv32im_bigint_accum_states_device(stream(), d_states, h_mix, h_backs, n, rows);
  });
}
const char* r0hip_rv32im_bigint_accum_inject(uint32_t* d_accum, size_t rows, const uint32_t* h_mix,
                                             const r0hip_bigint_back* h_backs, size_t n) {
  return wrap_dev([&] {
    R0_REQUIRE(d_accum && h_mix, "r0hip_rv32im_bigint_accum_inject: null argument");
    if (!deferred_mode()) stage_reset();  // it drains; the deferred arena recycles itself
    rv32im_bigint_inject(stream(), d_accum, rows, h_mix, h_backs, n);
  });
}
const char* r0hip_recursion_accum(const uint32_t* d_ctrl, const uint32_t* d_global, const uint32_t* d_data,
                                  const uint32_t* d_mix, uint32_t* d_accum, size_t work_cycles,
                                  size_t total_cycles) {
  return wrap_dev([&] {
    R0_REQUIRE(d_ctrl && d_global && d_data && d_mix && d_accum, "r0hip_recursion_accum: null argument");
    recursion_accum(stream(), d_ctrl, d_global, d_data, d_mix, d_accum, work_cycles, total_cycles);
  });
}
const char* r0hip_rv32im_witgen(uint32_t mode, const r0hip_raw_exec_buffers* buffers,
                                const r0hip_raw_preflight_trace* preflight, uint32_t cycles) {
  return wrap([&] {
    R0_REQUIRE(buffers && preflight && buffers->global.buf && buffers->data.buf, "r0hip_rv32im_witgen: null argument");
    const CircuitDef* c = find_circuit("rv32im");
    R0_REQUIRE(buffers->data.cols == c->group_size(2) && buffers->global.cols == c->output_size &&
                   buffers->global.rows == 1,
               "r0hip_rv32im_witgen: buffers are not the rv32im data group and global vector");
    R0_REQUIRE(cycles == buffers->data.rows, "r0hip_rv32im_witgen: cycles must equal the data group's rows");
    // the reference's witness generator takes Buffer<checked = true> (witgen/mod.rs:150) and
    // these kernels always run the checked stores and reads
    R0_REQUIRE(buffers->data.checked && buffers->global.checked,
               "r0hip_rv32im_witgen: unchecked buffers are not supported (the reference passes checked = true)");
    stage_reset();
    rv32im_witgen(stream(), mode, buffers->data.buf, buffers->global.buf, buffers->data.rows,
                  static_cast<const rvwg::PreflightCycle*>(preflight->cycles),
                  static_cast<const rvwg::MemoryTxn*>(preflight->txns), preflight->txns_len, preflight->bigint_bytes,
                  preflight->bigint_bytes_len, preflight->table_split_cycle, cycles);
  });
}

}  // extern "C"

// A recursion program resident on the device (r0hip_recursion_program_*): the control group
// WitnessGenerator::new lays out (witgen.rs:57-67) and its commitment, which depend only on
// (program, po2, suite), made once. The four buffers are dedicated allocations, read-only after
// create; `top` is the host copy of the tree's root and top layers, control_id the root
// (Program::compute_control_id, program.rs:74-104).
struct r0hip_recursion_program {
  static constexpr uint64_t kDestroyed = ~uint64_t(0);
  int suite = 0;
  uint32_t po2 = 0;
  size_t code_rows = 0;
  uint32_t* buf[4] = {nullptr, nullptr, nullptr, nullptr};  // ctrl, coeffs, evaluated, nodes
  size_t bytes[4] = {0, 0, 0, 0};
  uint32_t control_id[8] = {};
  std::vector<uint32_t> top;
  mutable std::atomic<uint64_t> uses{0};  // proofs running and worker jobs queued
  // r0hip_recursion_program_prepare_input: the op table and fixed tables on the host, the witness
  // generator's plan on the device; written once under plan_mu, read-only once `planned` is set
  mutable std::mutex plan_mu;
  mutable std::atomic<bool> planned{false};
  mutable r0::rpf::Program ops;
  mutable r0::RecursionWitgenPlan plan;
  ~r0hip_recursion_program() {
    for (int i = 0; i < 4; i++) dev_free_dedicated(buf[i], bytes[i]);
    r0::recursion_witgen_plan_free(&plan);
  }
};

namespace r0 {

void check_injector(const uint32_t* index, size_t rows, const uint32_t* offsets, const uint32_t* values,
                    size_t limit, size_t seg_rows);

// r0hip_backs on the host (backs.h)
BacksInfo check_backs(const r0hip_backs* b, size_t seg_rows, const std::string& who) {
  R0_REQUIRE(b, who + ": backs is NULL");
  R0_REQUIRE(b->inj_rows <= seg_rows, who + ": backs: inj_rows " + std::to_string(b->inj_rows) + " above the segment's " +
                                          std::to_string(seg_rows) + " rows");
  R0_REQUIRE(b->n == 0 || b->recs, who + ": backs: recs is NULL with " + std::to_string(b->n) + " records");
  R0_REQUIRE(b->n_words == 0 || b->words, who + ": backs: words is NULL with n_words " + std::to_string(b->n_words));
  R0_REQUIRE(b->n_words < (size_t(1) << 32), who + ": backs: n_words does not fit a record's 32-bit word index");
  const rvwg::BackTables& T = rv32im_witgen_back_tables();
  BacksInfo info;
  for (size_t k = 0; k < b->n; k++) {
    const r0hip_back& r = b->recs[k];
    auto rec = [&] { return who + ": backs: record " + std::to_string(k) + " (row " + std::to_string(r.row) + ")"; };
    R0_REQUIRE(r.row < b->inj_rows, rec() + ": row at or past inj_rows " + std::to_string(b->inj_rows));
    R0_REQUIRE(k == 0 || r.row > b->recs[k - 1].row,
               rec() + ": rows must strictly increase (the record before it has row " +
                   std::to_string(k ? b->recs[k - 1].row : 0) + ")");
    R0_REQUIRE(r.kind >= 1 && r.kind < rvwg::kBackKinds, rec() + ": kind " + std::to_string(r.kind) + " is not 1..4");
    const size_t size = size_t(T.plain[r.kind]) + T.bits[r.kind];
    R0_REQUIRE(size_t(r.word) + size <= b->n_words, rec() + ": payload words [" + std::to_string(r.word) + ", " +
                                                        std::to_string(size_t(r.word) + size) + ") end past n_words " +
                                                        std::to_string(b->n_words));
    info.entries += size_t(T.plain[r.kind]) + 32 * size_t(T.bits[r.kind]);
    info.n_bigint += r.kind == R0HIP_BACK_BIGINT;
  }
  return info;
}

std::vector<r0hip_bigint_back> backs_bigint_records(const r0hip_backs& b, size_t n_bigint) {
  std::vector<r0hip_bigint_back> out;
  out.reserve(n_bigint);
  for (size_t k = 0; k < b.n && n_bigint; k++) {
    if (b.recs[k].kind != R0HIP_BACK_BIGINT) continue;
    const uint32_t* w = b.words + b.recs[k].word;  // is_ecall, mode, pc, poly_op, coeff, bytes[16], next_state
    r0hip_bigint_back r{};
    r.row = b.recs[k].row;
    r.poly_op = w[3];
    r.coeff = w[4];
    for (int i = 0; i < 16; i++) r.bytes[i] = uint8_t(w[5 + i]);
    out.push_back(r);
  }
  return out;
}

// SegmentProverImpl::prove_core from a preflight (circuit/rv32im/src/prove/hal/mod.rs:143-224):
// WitnessGenerator::hal_generate_witness (witgen/mod.rs:135-176: globals, code and data
// INVALID, the injector scattered into data, stepExec, zeroize), then the prove core with the
// version word 2 and WitnessGenerator::accum on the device. `resident`: the global vector,
// the injector and the preflight arrays are device pointers; otherwise host pointers.
// inputs_ready (resident only): called with the stream after the groups' fill (which reads no
// input) and before the first read of the inputs (the segment pipeline makes the stream wait for
// their upload there, so the fill runs while the trace still uploads).
// backs: the injector as checked Back records (backs.h) instead of the inj_* arrays, which are
// then not read; its arrays are device pointers when `resident`.
std::vector<uint32_t> prove_trace(int suite, uint32_t po2, uint32_t mode, const uint32_t* global_in,
                                  const uint32_t* inj_index, size_t inj_rows, const uint32_t* inj_offsets,
                                  const uint32_t* inj_values, const r0hip_raw_preflight_trace* pf,
                                  const r0hip_bigint_back* h_bigint, size_t n_bigint, bool resident,
                                  std::vector<uint32_t>* mix, const std::function<void(hipStream_t)>& inputs_ready,
                                  const TraceBacks* backs) {
  const CircuitDef* c = find_circuit("rv32im");
  if (backs) inj_rows = backs->inj_rows;
  R0_REQUIRE(global_in && (inj_index || backs) && pf && pf->cycles, "r0hip_prove_segment_trace: null argument");
  R0_REQUIRE(po2 >= 2 && po2 <= 24, "r0hip_prove_segment_trace: po2 out of range");
  R0_REQUIRE(n_bigint == 0 || h_bigint, "r0hip_prove_segment_trace: h_bigint is NULL with n_bigint > 0");
  const size_t n = size_t(1) << po2;
  R0_REQUIRE(inj_rows <= n, "r0hip_prove_segment_trace: injector longer than the segment");
  const size_t data_cols = c->group_size(2);
  hipStream_t s = stream();
  stage_reset();
  Span span("prove_segment_trace");
  DevBuf code(c->group_size(1) * n), data(data_cols * n), global(c->output_size), accum(c->group_size(0) * n);
  // the groups as WitnessGenerator::new / ::accum allocate them (INVALID), already zeroized where
  // nothing reads INVALID (rv32im_prover_groups_fill), then the injector (rv32im_prover_inject)
  rv32im_prover_groups_fill(s, data.p, code.p, accum.p, n, c->group_size(0));
  const uint32_t *idx = inj_index, *off = inj_offsets, *val = inj_values;
  const uint32_t *recs = backs ? backs->recs : nullptr, *words = backs ? backs->words : nullptr;
  const rvwg::PreflightCycle* cyc = static_cast<const rvwg::PreflightCycle*>(pf->cycles);
  const rvwg::MemoryTxn* txn = static_cast<const rvwg::MemoryTxn*>(pf->txns);
  const uint8_t* big = pf->bigint_bytes;
  if (resident) {
    if (inputs_ready) inputs_ready(s);
    HIP_OK(hipMemcpyAsync(global.p, global_in, global.words * 4, hipMemcpyDeviceToDevice, s));
  } else {
    R0_REQUIRE((pf->txns_len == 0 || pf->txns) && (pf->bigint_bytes_len == 0 || pf->bigint_bytes),
               "r0hip_prove_segment_trace: null trace array with a nonzero count");
    upload_async(global.p, global_in, global.words * 4);
    if (backs) {  // checked by the caller (check_backs)
      auto* d_recs = static_cast<uint32_t*>(scratch(backs->n * 12 + 4, kSlotRvBackRecs));
      auto* d_words = static_cast<uint32_t*>(scratch(backs->n_words * 4 + 4, kSlotRvBackWords));
      upload_async(d_recs, backs->recs, backs->n * 12);
      upload_async(d_words, backs->words, backs->n_words * 4);
      recs = d_recs, words = d_words;
    } else {
      check_injector(inj_index, inj_rows, inj_offsets, inj_values, data_cols * n, n);
      const size_t n_inj = inj_index[inj_rows];
      auto* d_idx = static_cast<uint32_t*>(scratch((inj_rows + 1) * 4, kSlotRvInjIndex));
      auto* d_off = static_cast<uint32_t*>(scratch(n_inj * 4 + 4, kSlotRvInjOffsets));
      auto* d_val = static_cast<uint32_t*>(scratch(n_inj * 4 + 4, kSlotRvInjValues));
      upload_async(d_idx, inj_index, (inj_rows + 1) * 4);
      upload_async(d_off, inj_offsets, n_inj * 4);
      upload_async(d_val, inj_values, n_inj * 4);
      idx = d_idx, off = d_off, val = d_val;
    }
    cyc = rv32im_upload_cycles(cyc, n);
    auto* d_txn = static_cast<rvwg::MemoryTxn*>(scratch(size_t(pf->txns_len) * sizeof(rvwg::MemoryTxn) + 16, kSlotRvwgTxns));
    auto* d_big = static_cast<uint8_t*>(scratch(size_t(pf->bigint_bytes_len) + 16, kSlotRvwgBigint));
    upload_async(d_txn, pf->txns, size_t(pf->txns_len) * sizeof(rvwg::MemoryTxn));
    upload_async(d_big, pf->bigint_bytes, pf->bigint_bytes_len);
    txn = pf->txns_len ? d_txn : nullptr;
    big = pf->bigint_bytes_len ? d_big : nullptr;
  }
  auto* ierr = static_cast<uint32_t*>(scratch(16, kSlotRvInitErr));
  HIP_OK(hipMemsetD32Async(ierr, 0u, 4, s));
  // the injector: the CSR list scattered, or the Back records expanded (the same words)
  auto inject = [&](uint32_t* err) {
    if (backs)
      rv32im_inject_backs(s, data.p, n, cyc, inj_rows, recs, backs->n, words, backs->n_words, backs->entries, err);
    else if (err)
      rv32im_prover_inject(s, data.p, n, idx, off, val, inj_rows, data.words, cyc, err);
    else
      scatter(s, data.p, idx, off, val, inj_rows, data.words);
  };
  inject(ierr);
  {
    Span w("witgen");
    // an injector entry outside its row's injected columns: the group as the reference prepares
    // it (hal_generate_witness, witgen/mod.rs:146-162), every word INVALID and the injector scattered
    auto reinit = [&] {
      HIP_OK(hipMemsetD32Async(data.p, 0xFFFFFFFFu, data.words, s));
      inject(nullptr);
    };
    rv32im_witgen_dev(s, mode, data.p, global.p, n, cyc, txn, pf->txns_len, big, pf->bigint_bytes_len,
                      pf->table_split_cycle, uint32_t(n), true, ierr, reinit);
  }
  eltwise_zeroize(s, global.p, global.words);  // the data group was zeroized by the witgen merge
  AccumStep acc{accum.p, n, false, h_bigint, n_bigint};
  acc.zeroed = true;
  return prove_segment(*c, suite, po2, code.p, data.p, nullptr, global.p, true, 2, mix, nullptr, &acc);
}

// The host injector (Injector, witgen/mod.rs:329-378) before it is uploaded: a CSR index that
// never decreases (entries of row c are [index[c], index[c + 1])), offsets inside the data group
// and in the entry's own row (col * seg_rows + c: Injector::set writes only its row). O(rows +
// entries); the resident path's inject pass bounds its reads and writes and reports other rows.
void check_injector(const uint32_t* index, size_t rows, const uint32_t* offsets, const uint32_t* values,
                    size_t limit, size_t seg_rows) {
  for (size_t c = 0; c < rows; c++)
    R0_REQUIRE(index[c] <= index[c + 1], "r0hip_prove_segment_trace: injector index decreases at row " +
                                             std::to_string(c));
  const size_t n_inj = index[rows];
  R0_REQUIRE(n_inj == 0 || (offsets && values), "r0hip_prove_segment_trace: null injector arrays");
  for (size_t c = 0; c < rows; c++)
    for (size_t i = index[c]; i < index[c + 1]; i++) {
      R0_REQUIRE(offsets[i] < limit, "r0hip_prove_segment_trace: injector offset outside the data group");
      R0_REQUIRE(offsets[i] % seg_rows == c, "r0hip_prove_segment_trace: injector entry of row " + std::to_string(c) +
                                                 " sets word " + std::to_string(offsets[i]) +
                                                 " of another row (Injector::set writes its own row)");
    }
}

// RecursionProverImpl::prove from the program and its preflight (circuit/recursion/src/prove/
// mod.rs:160-230). noise(s, out, count, which) fills `count` words of the ZK noise matrix
// `which` (0 the data group's, 1 the accum group's) on stream s.
// witgen(s, data, global): the witness generator, called once the data group and the globals
// are INVALID words
using RecursionWitgen = std::function<void(hipStream_t s, uint32_t* data, uint32_t* global)>;
static std::vector<uint32_t> prove_recursion_with(int suite, uint32_t po2, const uint32_t* d_ctrl, size_t n_cycles,
                                                  const RecursionWitgen& witgen, const RecursionNoise& noise_fill,
                                                  std::vector<uint32_t>* mix, const CachedGroup* ctrl_cached) {
  const CircuitDef* c = find_circuit("recursion");
  R0_REQUIRE(c && d_ctrl, "r0hip_prove_recursion: null argument");
  R0_REQUIRE(po2 >= 11 && po2 <= 24, "r0hip_prove_recursion: po2 out of range (ZK rows need po2 >= 11)");
  constexpr size_t kZk = 1024;  // risc0_zkp::ZK_CYCLES (zkp/src/lib.rs:42)
  const size_t n = size_t(1) << po2;
  R0_REQUIRE(n_cycles <= n - kZk, "r0hip_prove_recursion: program longer than 2^po2 - ZK_CYCLES rows");
  const size_t data_cols = c->group_size(2), accum_cols = c->group_size(0);
  hipStream_t s = stream();
  stage_reset();
  // WitnessGenerator::new (circuit/recursion/src/prove/witgen.rs:44-133)
  DevBuf data(data_cols * n), global(c->output_size), accum(accum_cols * n), noise(std::max(data_cols, accum_cols) * kZk);
  // r0hip_set_proof_streams >= 2: the control group needs nothing of the witness generation, so
  // its NTTs and hashes (throughput work) run on a side stream beside the generator, which is
  // bound by the latency of its exec runs and waits for the host; prove_segment joins
  GroupWork code_early;
  // (a cached control group has no commit left to move)
  const bool early = !ctrl_cached && active_proof_streams() >= 2;
  if (early) code_early = commit_group_side(1, suite, d_ctrl, c->group_size(1), po2);
  HIP_OK(hipMemsetD32Async(data.p, 0xFFFFFFFFu, data.words, s));
  HIP_OK(hipMemsetD32Async(global.p, 0xFFFFFFFFu, global.words, s));
  witgen(s, data.p, global.p);
  // ZK noise in the last ZK_CYCLES data rows (witgen.rs:101-116: eltwise_copy_elem_slice
  // from a data_size x ZK_CYCLES noise matrix), per-cell values of the noise generator
  noise_fill(s, noise.p, data_cols * kZk, 0);
  copy_elem_slice(s, data.p, noise.p, data_cols, kZk, 0, kZk, n - kZk, n);
  eltwise_zeroize(s, data.p, data.words);
  // WitnessGenerator::accum (witgen.rs:134-177): INVALID plus noise rows, then the
  // accumulation inside the proof; prove (prove/mod.rs:160-230)
  HIP_OK(hipMemsetD32Async(accum.p, 0xFFFFFFFFu, accum.words, s));
  noise_fill(s, noise.p, accum_cols * kZk, 1);
  copy_elem_slice(s, accum.p, noise.p, accum_cols, kZk, 0, kZk, n - kZk, n);
  const AccumStep acc{accum.p, n_cycles};
  return prove_segment(*c, suite, po2, d_ctrl, data.p, nullptr, global.p, false, 0, mix, nullptr, &acc,
                       early ? &code_early : nullptr, ctrl_cached);
}

std::vector<uint32_t> prove_recursion(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom,
                                      size_t n_wom, const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                      size_t n_iops, const RecursionNoise& noise_fill, std::vector<uint32_t>* mix,
                                      const CachedGroup* ctrl_cached) {
  const size_t n = size_t(1) << (po2 <= 24 ? po2 : 0);
  return prove_recursion_with(
      suite, po2, d_ctrl, n_cycles,
      [&](hipStream_t s, uint32_t* data, uint32_t* global) {
        recursion_witgen(s, d_ctrl, data, global, n, h_wom, n_wom, h_cycles, n_cycles, h_iops, n_iops);
      },
      noise_fill, mix, ctrl_cached);
}

// The keyed noise of r0hip_prove_recursion_keyed: ChaCha20 under `key`, the data matrix with
// nonce {0, lo32(stream_id), hi32(stream_id)}, the accum matrix with {1, lo32, hi32}.
RecursionNoise keyed_noise(const uint32_t* key, uint64_t stream_id) {
  return [key, stream_id](hipStream_t s, uint32_t* out, size_t count, uint32_t which) {
    ChaChaKey k;
    memcpy(k.key, key, sizeof k.key);
    k.nonce[0] = which;
    k.nonce[1] = uint32_t(stream_id);
    k.nonce[2] = uint32_t(stream_id >> 32);
    fill_chacha20(s, out, count, k);
    explicit_bzero(&k, sizeof k);
  };
}

RecursionProgramShape recursion_program_shape(const r0hip_recursion_program* h) {
  return RecursionProgramShape{h->suite, h->po2, h->code_rows, h->control_id};
}
void recursion_program_acquire(const r0hip_recursion_program* h) {
  uint64_t v = h->uses.load(std::memory_order_relaxed);
  do {
    R0_REQUIRE(v != r0hip_recursion_program::kDestroyed, "recursion program: the handle is being destroyed");
  } while (!h->uses.compare_exchange_weak(v, v + 1, std::memory_order_acquire, std::memory_order_relaxed));
}
void recursion_program_release(const r0hip_recursion_program* h) noexcept {
  h->uses.fetch_sub(1, std::memory_order_release);
}

// r0hip_prove_recursion_program: prove_recursion with the control group and its commitment taken
// from the handle (the caller holds a use count)
std::vector<uint32_t> prove_recursion_program(const r0hip_recursion_program* h, const uint32_t* h_wom, size_t n_wom,
                                              const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                              size_t n_iops, const RecursionNoise& noise_fill,
                                              std::vector<uint32_t>* mix) {
  // witgen.rs:80: the trace has one cycle per program row
  R0_REQUIRE(n_cycles == h->code_rows, "r0hip_prove_recursion_program: n_cycles " + std::to_string(n_cycles) +
                                           " is not the program's code_rows " + std::to_string(h->code_rows));
  const CachedGroup cg{h->buf[1], h->buf[2], h->buf[3], 23, h->top.data()};
  return prove_recursion(h->suite, h->po2, h->buf[0], h_wom, n_wom, h_cycles, n_cycles, h_iops, n_iops, noise_fill, mix,
                         &cg);
}

// host milliseconds of the preflight inside this thread's last prove_recursion_program_input
static thread_local double t_last_preflight_ms = 0;
double recursion_last_preflight_ms() { return t_last_preflight_ms; }

// r0hip_recursion_program_prepare_input. The control group comes back from the device (create
// keeps no host copy and stays as cheap as it was), is decoded once, and the witness generator's
// plan is made from the decoded {iopIdx, isParSafe}. A failure leaves the handle without a plan
// and the next call tries again.
RecursionInputCounts recursion_program_prepare_input(const r0hip_recursion_program* h) {
  if (!h->planned.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(h->plan_mu);
    if (!h->planned.load(std::memory_order_relaxed)) {
      const size_t n = size_t(1) << h->po2;
      std::vector<uint32_t> ctrl(23 * n);
      stage_reset();
      download(ctrl.data(), h->buf[0], ctrl.size() * 4);
      rpf::Program ops = rpf::decode_columns(ctrl.data(), h->code_rows, h->po2);
      recursion_witgen_plan(stream(), h->buf[0], n, ops.cycles.data(), h->code_rows, &h->plan);
      h->ops = std::move(ops);
      h->planned.store(true, std::memory_order_release);
    }
  }
  return RecursionInputCounts{h->ops.n_wom, h->ops.n_iops, h->ops.n_output};
}

bool recursion_program_planned_counts(const r0hip_recursion_program* h, RecursionInputCounts* out) {
  if (!h->planned.load(std::memory_order_acquire)) return false;
  *out = RecursionInputCounts{h->ops.n_wom, h->ops.n_iops, h->ops.n_output};
  return true;
}

void recursion_program_preflight_into(const r0hip_recursion_program* h, const uint32_t* h_input, size_t n_input,
                                      uint32_t* wom, uint32_t* iops, uint32_t* output) {
  rpf::run(h->ops, h_input, n_input, wom, iops, output);
}

std::vector<uint32_t> prove_recursion_program_input(const r0hip_recursion_program* h, const uint32_t* h_input,
                                                    size_t n_input, const uint32_t* h_wom, const uint32_t* h_iops,
                                                    uint32_t* output, const RecursionNoise& noise_fill,
                                                    std::vector<uint32_t>* mix) {
  const RecursionInputCounts cnt = recursion_program_prepare_input(h);
  const CachedGroup cg{h->buf[1], h->buf[2], h->buf[3], 23, h->top.data()};
  return prove_recursion_with(
      h->suite, h->po2, h->buf[0], h->code_rows,
      [&](hipStream_t s, uint32_t* data, uint32_t* global) {
        const uint32_t *wom = h_wom, *iops = h_iops;
        if (!wom) {
          // the preflight writes its upload in place (the group fills queued above run meanwhile)
          Span sp("preflight");
          auto* w = static_cast<uint32_t*>(stage_host(cnt.n_wom * 16 + 16));
          auto* i = static_cast<uint32_t*>(stage_host(cnt.n_iops * 16 + 16));
          const auto t0 = std::chrono::steady_clock::now();
          rpf::run(h->ops, h_input, n_input, w, i, output);
          t_last_preflight_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
          wom = w, iops = i;
        }
        recursion_witgen_planned(s, h->buf[0], data, global, size_t(1) << h->po2, h->plan, wom, cnt.n_wom, iops,
                                 cnt.n_iops, true);
      },
      noise_fill, mix, &cg);
}

void os_random_key(uint32_t key[8]) {
  auto* p = reinterpret_cast<uint8_t*>(key);
  for (size_t got = 0; got < 32;) {
    const ssize_t r = getrandom(p + got, 32 - got, 0);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) {
      explicit_bzero(key, 32);
      throw std::runtime_error(std::string("r0hip: getrandom failed: ") + strerror(errno));
    }
    got += size_t(r);
  }
}

}  // namespace r0

namespace {

void seal_out(const std::vector<uint32_t>& seal, const std::vector<uint32_t>& mix, uint32_t* h_seal, size_t seal_cap,
              size_t* seal_len, uint32_t* h_mix_out) {
  if (seal_len) *seal_len = seal.size();
  if (h_mix_out) memcpy(h_mix_out, mix.data(), mix.size() * 4);
  if (h_seal) {
    R0_REQUIRE(seal.size() <= seal_cap, "seal buffer too small");
    memcpy(h_seal, seal.data(), seal.size() * 4);
  }
}

}  // namespace

extern "C" {

const char* r0hip_prove_segment_trace(int suite, uint32_t po2, uint32_t mode, const uint32_t* h_global,
                                      const uint32_t* h_inj_index, size_t inj_rows, const uint32_t* h_inj_offsets,
                                      const uint32_t* h_inj_values, const r0hip_raw_preflight_trace* preflight,
                                      const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* h_seal,
                                      size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    std::vector<uint32_t> mix;
    auto seal = prove_trace(suite, po2, mode, h_global, h_inj_index, inj_rows, h_inj_offsets, h_inj_values, preflight,
                            h_bigint, n_bigint, false, &mix, {}, nullptr);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
}

const char* r0hip_prove_segment_trace_backs(int suite, uint32_t po2, uint32_t mode, const uint32_t* h_global,
                                            const r0hip_raw_preflight_trace* preflight, const r0hip_backs* backs,
                                            uint32_t* h_seal, size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    R0_REQUIRE(po2 >= 2 && po2 <= 24, "r0hip_prove_segment_trace_backs: po2 out of range");
    const BacksInfo info = check_backs(backs, size_t(1) << po2, "r0hip_prove_segment_trace_backs");
    const std::vector<r0hip_bigint_back> bigint = backs_bigint_records(*backs, info.n_bigint);
    const TraceBacks tb{reinterpret_cast<const uint32_t*>(backs->recs), backs->n, backs->words, backs->n_words,
                        backs->inj_rows, info.entries};
    std::vector<uint32_t> mix;
    auto seal = prove_trace(suite, po2, mode, h_global, nullptr, 0, nullptr, nullptr, preflight,
                            bigint.empty() ? nullptr : bigint.data(), bigint.size(), false, &mix, {}, &tb);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
}

const char* r0hip_rv32im_inject_backs(uint32_t* d_data, size_t rows, const void* h_cycles, const r0hip_backs* backs) {
  return wrap_dev([&] {
    R0_REQUIRE(d_data, "r0hip_rv32im_inject_backs: d_data is NULL");
    R0_REQUIRE(rows >= 4 && rows <= (size_t(1) << 24) && (rows & (rows - 1)) == 0,
               "r0hip_rv32im_inject_backs: rows must be a power of two in [4, 2^24]");
    const BacksInfo info = check_backs(backs, rows, "r0hip_rv32im_inject_backs");
    R0_REQUIRE(backs->inj_rows == 0 || h_cycles, "r0hip_rv32im_inject_backs: h_cycles is NULL");
    if (!deferred_mode()) stage_reset();  // it drains; the deferred arena recycles itself
    const rvwg::PreflightCycle* d_cycles =
        rv32im_upload_cycles(static_cast<const rvwg::PreflightCycle*>(h_cycles), backs->inj_rows);
    auto* d_recs = static_cast<uint32_t*>(scratch(backs->n * 12 + 4, kSlotRvBackRecs));
    auto* d_words = static_cast<uint32_t*>(scratch(backs->n_words * 4 + 4, kSlotRvBackWords));
    upload_async(d_recs, backs->recs, backs->n * 12);
    upload_async(d_words, backs->words, backs->n_words * 4);
    rv32im_inject_backs(stream(), d_data, rows, d_cycles, backs->inj_rows, d_recs, backs->n, d_words, backs->n_words,
                        info.entries, nullptr);
  });
}

const char* r0hip_prove_segment_trace_resident(int suite, uint32_t po2, uint32_t mode, const uint32_t* d_global,
                                               const uint32_t* d_inj_index, size_t inj_rows,
                                               const uint32_t* d_inj_offsets, const uint32_t* d_inj_values,
                                               const r0hip_raw_preflight_trace* d_preflight,
                                               const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* h_seal,
                                               size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    std::vector<uint32_t> mix;
    auto seal = prove_trace(suite, po2, mode, d_global, d_inj_index, inj_rows, d_inj_offsets, d_inj_values,
                            d_preflight, h_bigint, n_bigint, true, &mix, {}, nullptr);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
}

const char* r0hip_recursion_witgen(const uint32_t* d_ctrl, uint32_t* d_data, uint32_t* d_global, size_t total_cycles,
                                   const uint32_t* h_wom, size_t n_wom, const uint32_t* h_cycles, size_t n_cycles,
                                   const uint32_t* h_iops, size_t n_iops) {
  return wrap([&] {
    R0_REQUIRE(d_ctrl && d_data && d_global, "r0hip_recursion_witgen: null argument");
    stage_reset();
    recursion_witgen(stream(), d_ctrl, d_data, d_global, total_cycles, h_wom, n_wom, h_cycles, n_cycles, h_iops,
                     n_iops);
  });
}

const char* r0hip_prove_recursion(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom, size_t n_wom,
                                  const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops, size_t n_iops,
                                  uint64_t noise_seed, uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                  uint32_t* h_mix_out) {
  return wrap([&] {
    std::vector<uint32_t> mix;
    auto seal = prove_recursion(suite, po2, d_ctrl, h_wom, n_wom, h_cycles, n_cycles, h_iops, n_iops,
                                [noise_seed](hipStream_t s, uint32_t* out, size_t count, uint32_t which) {
                                  fill_uniform(s, out, count, noise_seed + which);
                                },
                                &mix);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
}

const char* r0hip_prove_recursion_keyed(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom,
                                        size_t n_wom, const uint32_t* h_cycles, size_t n_cycles,
                                        const uint32_t* h_iops, size_t n_iops, const uint32_t* h_key,
                                        uint64_t stream_id, uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                        uint32_t* h_mix_out) {
  uint32_t key[8];
  const char* err = wrap([&] {
    if (h_key) memcpy(key, h_key, sizeof key);
    else os_random_key(key);
    std::vector<uint32_t> mix;
    auto seal = prove_recursion(suite, po2, d_ctrl, h_wom, n_wom, h_cycles, n_cycles, h_iops, n_iops,
                                keyed_noise(key, stream_id), &mix);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
  explicit_bzero(key, sizeof key);
  return err;
}

const char* r0hip_recursion_program_create(r0hip_recursion_program** out, int suite, uint32_t po2,
                                           const uint32_t* h_code, size_t n_words, int form) {
  return wrap([&] {
    // every refusal on the host, before any device call
    const std::string who = "r0hip_recursion_program_create: ";
    R0_REQUIRE(out, who + "out is NULL");
    *out = nullptr;
    R0_REQUIRE(h_code, who + "h_code is NULL");
    R0_REQUIRE(suite >= 0 && suite <= 2, who + "suite " + std::to_string(suite) + " is not a hash suite (0..2)");
    R0_REQUIRE(form == R0HIP_CODE_ENCODED || form == R0HIP_CODE_MONTGOMERY,
               who + "form " + std::to_string(form) + " is neither R0HIP_CODE_ENCODED nor R0HIP_CODE_MONTGOMERY");
    R0_REQUIRE(po2 >= 11 && po2 <= 24, who + "po2 " + std::to_string(po2) + " outside 11..24 (the ZK rows need po2 >= 11)");
    R0_REQUIRE(n_words != 0, who + "n_words is 0");
    R0_REQUIRE(n_words % 23 == 0, who + "n_words " + std::to_string(n_words) + " is not a multiple of 23 (words per row)");
    const size_t n = size_t(1) << po2, rows = n_words / 23;
    R0_REQUIRE(rows <= n - 1024, who + "n_words gives " + std::to_string(rows) + " rows, above 2^po2 - ZK_CYCLES = " +
                                     std::to_string(n - 1024));
    if (form == R0HIP_CODE_MONTGOMERY)
      for (size_t i = 0; i < n_words; i++)
        R0_REQUIRE(h_code[i] < kP, who + "h_code[" + std::to_string(i) + "] = " + std::to_string(h_code[i]) +
                                       " is not a canonical Montgomery word (>= p)");
    auto h = std::make_unique<r0hip_recursion_program>();
    h->suite = suite;
    h->po2 = po2;
    h->code_rows = rows;
    const size_t words[4] = {23 * n, 23 * n, 23 * n * 4, n * 4 * 2 * 8};
    for (int i = 0; i < 4; i++) {
      h->buf[i] = static_cast<uint32_t*>(dev_alloc_dedicated(words[i] * 4));
      h->bytes[i] = words[i] * 4;
    }
    hipStream_t s = stream();
    stage_reset();
    DevBuf code(n_words);
    upload(code.p, h_code, n_words * 4);
    recursion_program_expand(s, h->buf[0], code.p, n_words, po2, form);
    h->top = commit_group_keep(s, suite, h->buf[1], h->buf[2], h->buf[3], h->buf[0], 23, po2);
    memcpy(h->control_id, h->top.data(), 32);
    *out = h.release();
  });
}

const char* r0hip_recursion_program_info(const r0hip_recursion_program* program, int* suite, uint32_t* po2,
                                         size_t* code_rows, uint32_t control_id[8], uint64_t* device_bytes) {
  return wrap_nosync([&] {
    R0_REQUIRE(program, "r0hip_recursion_program_info: program is NULL");
    if (suite) *suite = program->suite;
    if (po2) *po2 = program->po2;
    if (code_rows) *code_rows = program->code_rows;
    if (control_id) memcpy(control_id, program->control_id, 32);
    if (device_bytes) *device_bytes = program->bytes[0] + program->bytes[1] + program->bytes[2] + program->bytes[3];
  });
}

const char* r0hip_recursion_program_ctrl(const r0hip_recursion_program* program, const uint32_t** d_ctrl) {
  return wrap_nosync([&] {
    R0_REQUIRE(program, "r0hip_recursion_program_ctrl: program is NULL");
    R0_REQUIRE(d_ctrl, "r0hip_recursion_program_ctrl: d_ctrl is NULL");
    *d_ctrl = program->buf[0];
  });
}

const char* r0hip_prove_recursion_program(const r0hip_recursion_program* program, const uint32_t* h_wom, size_t n_wom,
                                          const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                          size_t n_iops, const uint32_t* h_key, uint64_t stream_id, uint32_t* h_seal,
                                          size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out) {
  uint32_t key[8];
  bool held = false;
  const char* err = wrap([&] {
    const std::string who = "r0hip_prove_recursion_program: ";
    R0_REQUIRE(program, who + "program is NULL");
    R0_REQUIRE(h_wom || !n_wom, who + "h_wom is NULL with n_wom " + std::to_string(n_wom));
    R0_REQUIRE(h_cycles || !n_cycles, who + "h_cycles is NULL with n_cycles " + std::to_string(n_cycles));
    R0_REQUIRE(h_iops || !n_iops, who + "h_iops is NULL with n_iops " + std::to_string(n_iops));
    R0_REQUIRE(!seal_cap || h_seal, who + "h_seal is NULL with seal_cap " + std::to_string(seal_cap));
    R0_REQUIRE(n_cycles == program->code_rows, who + "n_cycles " + std::to_string(n_cycles) +
                                                   " is not the program's code_rows " +
                                                   std::to_string(program->code_rows));
    recursion_program_acquire(program);
    held = true;
    if (h_key) memcpy(key, h_key, sizeof key);
    else os_random_key(key);
    std::vector<uint32_t> mix;
    auto seal = prove_recursion_program(program, h_wom, n_wom, h_cycles, n_cycles, h_iops, n_iops,
                                        keyed_noise(key, stream_id), &mix);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
  });
  // wrap has drained this thread's stream (on an error too): nothing of the proof reads the handle
  if (held) recursion_program_release(program);
  explicit_bzero(key, sizeof key);
  return err;
}

const char* r0hip_recursion_preflight(const uint32_t* h_code, size_t n_words, int form, uint32_t po2,
                                      const uint32_t* h_input, size_t n_input, uint32_t* h_wom, size_t wom_cap,
                                      size_t* n_wom, uint32_t* h_cycles, size_t cycles_cap, size_t* n_cycles,
                                      uint32_t* h_iops, size_t iops_cap, size_t* n_iops, uint32_t* h_output,
                                      size_t output_cap, size_t* n_output) {
  return wrap_nosync([&] {
    const std::string who = "r0hip_recursion_preflight: ";
    R0_REQUIRE(h_input || !n_input, who + "h_input is NULL with n_input " + std::to_string(n_input));
    const rpf::Program p = rpf::decode(h_code, n_words, form, po2);
    if (n_wom) *n_wom = p.n_wom;
    if (n_cycles) *n_cycles = p.ops.size();
    if (n_iops) *n_iops = p.n_iops;
    if (n_output) *n_output = p.n_output;
    if (!h_wom && !h_cycles && !h_iops && !h_output) return;  // the size query
    R0_REQUIRE(h_wom && h_cycles && h_iops && h_output, who + "pass every out array, or none for the size query");
    R0_REQUIRE(wom_cap >= p.n_wom && cycles_cap >= p.ops.size() && iops_cap >= p.n_iops && output_cap >= p.n_output,
               who + "an out array is too small: the program needs " + std::to_string(p.n_wom) + " WOM cells, " +
                   std::to_string(p.ops.size()) + " cycles, " + std::to_string(p.n_iops) + " IOP values and " +
                   std::to_string(p.n_output) + " output words");
    memcpy(h_cycles, p.cycles.data(), p.cycles.size() * 4);
    rpf::run(p, h_input, n_input, h_wom, h_iops, h_output);
  });
}

const char* r0hip_recursion_program_prepare_input(const r0hip_recursion_program* program) {
  bool held = false;
  const char* err = wrap([&] {
    R0_REQUIRE(program, "r0hip_recursion_program_prepare_input: program is NULL");
    recursion_program_acquire(program);
    held = true;
    recursion_program_prepare_input(program);
  });
  if (held) recursion_program_release(program);
  return err;
}

const char* r0hip_recursion_program_input_info(const r0hip_recursion_program* program, r0hip_recursion_input_info* out) {
  return wrap_nosync([&] {
    R0_REQUIRE(program && out, "r0hip_recursion_program_input_info: null argument");
    *out = r0hip_recursion_input_info{};
    if (!program->planned.load(std::memory_order_acquire)) return;
    const rpf::Program& p = program->ops;
    out->prepared = 1;
    out->n_runs = program->plan.nruns;
    for (int k = 0; k < 9; k++) out->bucket_runs[k] = program->plan.counts[k];
    out->n_wom = p.n_wom;
    out->n_iops = p.n_iops;
    out->n_output = p.n_output;
    out->n_input = p.n_input;
    out->plan_device_bytes = program->plan.bytes;
    out->plan_host_bytes = p.ops.size() * sizeof(rpf::Op) + p.cycles.size() * 4;
  });
}

const char* r0hip_recursion_last_preflight_ms(double* out) {
  return wrap_nosync([&] {
    R0_REQUIRE(out, "r0hip_recursion_last_preflight_ms: out is NULL");
    *out = recursion_last_preflight_ms();
  });
}

const char* r0hip_prove_recursion_program_input(const r0hip_recursion_program* program, const uint32_t* h_input,
                                                size_t n_input, const uint32_t* h_key, uint64_t stream_id,
                                                uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                                uint32_t* h_mix_out, uint32_t* h_output, size_t output_cap,
                                                size_t* n_output) {
  uint32_t key[8];
  bool held = false;
  const char* err = wrap([&] {
    const std::string who = "r0hip_prove_recursion_program_input: ";
    R0_REQUIRE(program, who + "program is NULL");
    R0_REQUIRE(h_input || !n_input, who + "h_input is NULL with n_input " + std::to_string(n_input));
    R0_REQUIRE(!seal_cap || h_seal, who + "h_seal is NULL with seal_cap " + std::to_string(seal_cap));
    R0_REQUIRE(!output_cap || h_output, who + "h_output is NULL with output_cap " + std::to_string(output_cap));
    recursion_program_acquire(program);
    held = true;
    const RecursionInputCounts cnt = recursion_program_prepare_input(program);
    if (n_output) *n_output = cnt.n_output;
    R0_REQUIRE(!h_output || cnt.n_output <= output_cap, who + "output buffer too small: the program writes " +
                                                            std::to_string(cnt.n_output) + " words");
    std::vector<uint32_t> output(cnt.n_output);
    if (h_key) memcpy(key, h_key, sizeof key);
    else os_random_key(key);
    std::vector<uint32_t> mix;
    auto seal = prove_recursion_program_input(program, h_input, n_input, nullptr, nullptr, output.data(),
                                              keyed_noise(key, stream_id), &mix);
    seal_out(seal, mix, h_seal, seal_cap, seal_len, h_mix_out);
    if (h_output && cnt.n_output) memcpy(h_output, output.data(), cnt.n_output * 4);
  });
  if (held) recursion_program_release(program);
  explicit_bzero(key, sizeof key);
  return err;
}

const char* r0hip_recursion_program_destroy(r0hip_recursion_program* program) {
  return wrap([&] {
    R0_REQUIRE(program, "r0hip_recursion_program_destroy: program is NULL");
    uint64_t idle = 0;
    R0_REQUIRE(program->uses.compare_exchange_strong(idle, r0hip_recursion_program::kDestroyed),
               "r0hip_recursion_program_destroy: program is in use by " + std::to_string(idle) +
                   " proofs or queued worker jobs; nothing was freed");
    delete program;
  });
}

const char* r0hip_fill_chacha20(uint32_t* d_out, size_t count, const uint32_t* h_key, const uint32_t* h_nonce) {
  ChaChaKey k;
  const char* err = wrap_dev([&] {
    R0_REQUIRE((d_out || !count) && h_key && h_nonce, "r0hip_fill_chacha20: null argument");
    memcpy(k.key, h_key, sizeof k.key);
    memcpy(k.nonce, h_nonce, sizeof k.nonce);
    fill_chacha20(stream(), d_out, count, k);
  });
  explicit_bzero(&k, sizeof k);
  return err;
}

const char* r0hip_fill_uniform(uint32_t* d_out, size_t count, uint64_t seed) {
  return wrap_dev([&] { fill_uniform(stream(), d_out, count, seed); });
}

const char* r0hip_hash_rows(int suite, uint32_t* d_out, const uint32_t* d_matrix, size_t rows, size_t cols) {
  return wrap_dev([&] {
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    hash_rows(stream(), suite, d_out, d_matrix, rows, cols);
  });
}
const char* r0hip_hash_fold(int suite, uint32_t* d_io, size_t input_size, size_t output_size) {
  return wrap_dev([&] {
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    hash_fold(stream(), suite, d_io, input_size, output_size);
  });
}
const char* r0hip_merkle_tree(int suite, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols) {
  return wrap_dev([&] {
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    R0_REQUIRE(rows > 0 && (rows & (rows - 1)) == 0, "merkle_tree: rows must be a power of two");
    merkle_tree(stream(), suite, d_nodes, d_matrix, rows, cols);
  });
}

const char* r0hip_eval_check(const char* circuit, uint32_t* d_check, const uint32_t* const* d_groups,
                             const uint32_t* d_mix, const uint32_t* d_global, const uint32_t* h_poly_mix,
                             uint32_t po2) {
  return wrap([&] {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(d_check && d_groups && h_poly_mix, "eval_check: null argument");
    for (int g = 0; g < 3; g++) R0_REQUIRE(d_groups[g], "eval_check: null register group");
    stage_reset();
    run_eval_check(*c, d_check, d_groups, d_mix, d_global, fe(h_poly_mix), po2);
  });
}

const char* r0hip_constraint_rows(const char* circuit, uint32_t po2, const uint32_t* d_code, const uint32_t* d_data,
                                  const uint32_t* d_accum, const uint32_t* d_mix, const uint32_t* d_global,
                                  const uint32_t* h_poly_mix, uint32_t* d_out, r0hip_constraint_report* report) {
  return wrap([&] {
    // every refusal on the host, before any device call
    const std::string who = "r0hip_constraint_rows: ";
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, who + unknown_circuit(circuit));
    R0_REQUIRE(po2 >= 2 && po2 <= 24, who + "po2 " + std::to_string(po2) + " out of range (2..24)");
    R0_REQUIRE(d_code, who + "d_code is NULL");
    R0_REQUIRE(d_data, who + "d_data is NULL");
    R0_REQUIRE(d_accum, who + "d_accum is NULL");
    R0_REQUIRE(d_mix, who + "d_mix is NULL");
    R0_REQUIRE(d_global, who + "d_global is NULL");
    R0_REQUIRE(report, who + "report is NULL");
    const FpExt poly_mix = constraint_rows_poly_mix(h_poly_mix);
    stage_reset();
    const uint32_t* groups[3] = {d_accum, d_code, d_data};
    constraint_rows_run(*c, po2, groups, d_mix, d_global, nullptr, nullptr, poly_mix, d_out, report);
  });
}

const char* r0hip_prove_segment(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                const uint32_t* d_data, const uint32_t* d_accum, uint32_t* d_global,
                                int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    std::vector<uint32_t> mix;
    std::vector<uint32_t> seal = prove_segment(*c, suite, po2, d_code, d_data, d_accum, d_global, write_version != 0,
                                               version, &mix);
    if (seal_len) *seal_len = seal.size();
    if (h_mix_out) memcpy(h_mix_out, mix.data(), mix.size() * 4);
    if (h_seal) {
      R0_REQUIRE(seal.size() <= seal_cap, "seal buffer too small");
      memcpy(h_seal, seal.data(), seal.size() * 4);
    }
  });
}

const char* r0hip_prove_segment_accum(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                      const uint32_t* d_data, uint32_t* d_accum, size_t work_cycles,
                                      const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* d_global,
                                      int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                      size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(n_bigint == 0 || h_bigint, "prove_segment_accum: h_bigint is NULL with n_bigint > 0");
    std::vector<uint32_t> mix;
    const AccumStep acc{d_accum, work_cycles, false, h_bigint, n_bigint};
    std::vector<uint32_t> seal = prove_segment(*c, suite, po2, d_code, d_data, nullptr, d_global, write_version != 0,
                                               version, &mix, nullptr, &acc);
    if (seal_len) *seal_len = seal.size();
    if (h_mix_out) memcpy(h_mix_out, mix.data(), mix.size() * 4);
    if (h_seal) {
      R0_REQUIRE(seal.size() <= seal_cap, "seal buffer too small");
      memcpy(h_seal, seal.data(), seal.size() * 4);
    }
  });
}

const char* r0hip_prove_segment_cb(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                   const uint32_t* d_data, r0hip_accum_fn accum, void* user, uint32_t* d_global,
                                   int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                   size_t* seal_len, uint32_t* h_mix_out) {
  return wrap([&] {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(accum, "r0hip_prove_segment_cb: accum is NULL");
    R0_REQUIRE(d_code && d_data && d_global, "r0hip_prove_segment_cb: null group");
    std::vector<uint32_t> mix;
    const AccumCallback cb{accum, user};
    std::vector<uint32_t> seal =
        prove_segment_cb(*c, suite, po2, d_code, d_data, d_global, write_version != 0, version, &mix, cb);
    if (seal_len) *seal_len = seal.size();
    if (h_mix_out) memcpy(h_mix_out, mix.data(), mix.size() * 4);
    if (h_seal) {
      R0_REQUIRE(seal.size() <= seal_cap, "seal buffer too small");
      memcpy(h_seal, seal.data(), seal.size() * 4);
    }
  });
}

const char* r0hip_circuit_info(const char* circuit, r0hip_circuit_desc* out, size_t out_size, char* names,
                               size_t names_cap) {
  return wrap_nosync([&] {
    std::string text;
    if (!circuit) {
      for (size_t i = 0; i < circuit_count(); i++) text += (i ? " " : "") + std::string(circuit_at(i).name);
      R0_REQUIRE(names, "r0hip_circuit_info: names is NULL with no circuit named");
    } else {
      const CircuitDef* c = find_circuit(circuit);
      R0_REQUIRE(c, "r0hip_circuit_info: " + unknown_circuit(circuit));
      R0_REQUIRE(out, "r0hip_circuit_info: out is NULL");
      R0_REQUIRE(out_size == sizeof(r0hip_circuit_desc),
                 "r0hip_circuit_info: out_size " + std::to_string(out_size) + " is not sizeof(r0hip_circuit_desc) = " +
                     std::to_string(sizeof(r0hip_circuit_desc)));
      for (int g = 0; g < 3; g++) out->group_sizes[g] = uint32_t(c->group_size(g));
      out->mix_size = uint32_t(c->mix_size);
      out->output_size = uint32_t(c->output_size);
      out->n_taps = uint32_t(c->n_taps);
      memcpy(out->info, c->circuit_info, 16);
      text = c->name;
    }
    if (names) {
      R0_REQUIRE(text.size() < names_cap, "r0hip_circuit_info: names_cap " + std::to_string(names_cap) +
                                              " is too small for " + std::to_string(text.size() + 1) + " bytes");
      memcpy(names, text.c_str(), text.size() + 1);
    }
  });
}

const char* r0hip_demo_witness(uint32_t po2, size_t n_active, uint32_t a0, uint32_t b0, uint32_t* d_code,
                               uint32_t* d_data, uint32_t* d_global) {
  return wrap_dev([&] { demo_witness(stream(), po2, n_active, a0, b0, d_code, d_data, d_global); });
}

const char* r0hip_demo_accum(uint32_t po2, size_t n_active, const uint32_t* d_data, const uint32_t* h_mix,
                             uint32_t* d_accum) {
  return wrap_dev([&] { demo_accum(stream(), po2, n_active, d_data, h_mix, d_accum); });
}

}  // extern "C"

namespace {
// r0hip_selftest, one suite: the three checks, each timed; `why` names the first that failed
struct DemoAccumArgs {
  uint32_t po2;
  size_t n;
  const uint32_t* data;
};
const char* demo_accum_cb(void* user, const uint32_t* h_mix, uint32_t* d_accum, void* s) {
  const DemoAccumArgs& a = *static_cast<const DemoAccumArgs*>(user);
  demo_accum(static_cast<hipStream_t>(s), a.po2, a.n, a.data, h_mix, d_accum);  // a throw fails the proof as well
  return nullptr;
}
// an error string of an extern "C" entry point as a std::string ("" = none), freed
std::string take(const char* err) {
  if (!err) return "";
  std::string m = err;
  free(const_cast<char*>(err));
  return m;
}
void selftest_suite(const CircuitDef& c, int suite, uint32_t po2, r0hip_selftest_suite& rep, std::string& why) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  auto fail = [&](const std::string& m) {
    if (why.empty()) why = "suite " + std::to_string(suite) + ": " + m;
  };
  hipStream_t s = stream();
  const size_t rows = size_t(1) << po2, n = rows - rows / 8;  // the top eighth stands for the ZK rows
  DevBuf code(3 * rows), data(3 * rows), global(3);
  // a: witness, proof, both verifiers. The noise key is fixed: the run is the same every time.
  auto t0 = clk::now();
  ChaChaKey key{};
  for (int i = 0; i < 8; i++) key.key[i] = 0x52304850u + uint32_t(i);
  key.nonce[0] = uint32_t(suite);
  fill_chacha20(s, data.p, 3 * rows, key);
  demo_witness(s, po2, n, fp_encode(1), fp_encode(1), code.p, data.p, global.p);
  DemoAccumArgs args{po2, n, data.p};
  std::vector<uint32_t> mix;
  std::vector<uint32_t> seal =
      prove_segment_cb(c, suite, po2, code.p, data.p, global.p, false, 0, &mix, AccumCallback{demo_accum_cb, &args});
  rep.seal_len = uint32_t(seal.size());
  uint32_t got = 0;
  std::string e = take(r0hip_verify_seal(c.name, suite, seal.data(), seal.size(), nullptr, 0, nullptr, &got));
  if (e.empty() && got != po2) e = "the seal verifies at po2 " + std::to_string(got);
  if (e.empty())
    e = take(r0hip_verify_seal_on(R0HIP_VERIFY_DEVICE, c.name, suite, seal.data(), seal.size(), nullptr, 0, nullptr, &got));
  if (e.empty()) rep.passed |= 1u;
  else fail("a: the proof of the demo witness is not accepted: " + e);
  rep.ms[0] = ms_since(t0);
  // b: the rows check on the witness as proved, then with a[r] changed: rows r and r + 1 tap it
  t0 = clk::now();
  {
    stage_reset();
    DevBuf accum(4 * rows), dmix(4);
    HIP_OK(hipMemsetD32Async(accum.p, 0xFFFFFFFFu, 4 * rows, s));
    demo_accum(s, po2, n, data.p, mix.data(), accum.p);
    eltwise_zeroize(s, accum.p, 4 * rows);
    upload_async(dmix.p, mix.data(), 16);
    const uint32_t* groups[3] = {accum.p, code.p, data.p};
    const FpExt pm = constraint_rows_poly_mix(nullptr);
    r0hip_constraint_report cr;
    constraint_rows_run(c, po2, groups, dmix.p, global.p, mix.data(), nullptr, pm, nullptr, &cr);
    bool ok = cr.bad_rows == 0;
    if (!ok) fail("b: " + std::to_string(cr.bad_rows) + " rows of the demo witness violate a constraint, first " +
                  std::to_string(cr.first_row));
    const uint32_t r = uint32_t(n / 2);
    uint32_t word = 0;
    download(&word, data.p + r, 4);
    word = fp_add(word, kOne);
    upload(data.p + r, &word, 4);
    constraint_rows_run(c, po2, groups, dmix.p, global.p, mix.data(), nullptr, pm, nullptr, &cr);
    if (ok && !(cr.bad_rows == 2 && cr.n_rows == 2 && cr.rows[0] == r && cr.rows[1] == r + 1 && cr.first_row == r)) {
      ok = false;
      fail("b: a changed word in row " + std::to_string(r) + " is reported as " + std::to_string(cr.bad_rows) +
           " bad rows, first " + std::to_string(cr.first_row));
    }
    if (ok) rep.passed |= 2u;
  }
  rep.ms[1] = ms_since(t0);
  // c: one changed seal word is a rejection
  t0 = clk::now();
  if (!seal.empty()) {
    seal[seal.size() / 2] ^= 1u;
    e = take(r0hip_verify_seal(c.name, suite, seal.data(), seal.size(), nullptr, 0, nullptr, &got));
    if (!e.empty()) rep.passed |= 4u;
    else fail("c: the verifier accepts a seal with word " + std::to_string(seal.size() / 2) + " changed");
  }
  rep.ms[2] = ms_since(t0);
}
}  // namespace

extern "C" {

const char* r0hip_selftest(uint32_t suites_mask, uint32_t po2, r0hip_selftest_report* out, size_t out_size) {
  return wrap([&] {
    const std::string who = "r0hip_selftest: ";
    R0_REQUIRE(suites_mask >= 1 && suites_mask <= 7,
               who + "suites_mask " + std::to_string(suites_mask) + " names no suite of bits 0..2");
    R0_REQUIRE(po2 >= 8 && po2 <= 24, who + "po2 " + std::to_string(po2) + " out of range (8..24)");
    R0_REQUIRE(out, who + "out is NULL");
    R0_REQUIRE(out_size == sizeof(r0hip_selftest_report),
               who + "out_size " + std::to_string(out_size) + " is not sizeof(r0hip_selftest_report) = " +
                   std::to_string(sizeof(r0hip_selftest_report)));
    const CircuitDef* c = find_circuit("demo");
    R0_REQUIRE(c, who + unknown_circuit("demo"));
    memset(out, 0, sizeof *out);
    std::string why;
    for (int suite = 0; suite < 3; suite++)
      if ((suites_mask >> suite) & 1) selftest_suite(*c, suite, po2, out->suite[suite], why);
    R0_REQUIRE(why.empty(), who + why);
  });
}

const char* r0hip_set_kernel_timing(int on) {
  return wrap([&] { ktimer_enable(on != 0); });
}

const char* r0hip_kernel_times(char* buf, size_t cap) {
  return wrap([&] {
    std::string p = ktimer_report();
    if (buf && cap) {
      strncpy(buf, p.c_str(), cap - 1);
      buf[cap - 1] = 0;
    }
  });
}

const char* r0hip_last_profile(char* buf, size_t cap) {
  return wrap([&] {
    std::string p = last_profile();
    if (buf && cap) {
      strncpy(buf, p.c_str(), cap - 1);
      buf[cap - 1] = 0;
    }
  });
}

// MemoryTracker (zkp/src/hal/mod.rs:292-317): out[0..5) = live bytes, peak live bytes,
// reserved bytes, peak reserved bytes, hipMalloc calls so far. Host-only, never fails.
const char* r0hip_mem_stats(uint64_t* out) {
  return wrap_nosync([&] {
    R0_REQUIRE(out != nullptr, "r0hip_mem_stats: null output");
    const MemStats m = mem_stats();
    out[0] = m.live;
    out[1] = m.peak_live;
    out[2] = m.reserved;
    out[3] = m.peak_reserved;
    out[4] = m.mallocs;
  });
}

const char* r0hip_mem_reset_peak(void) {
  return wrap_nosync([&] { mem_reset_peak(); });
}

const char* r0hip_trim(void) {
  return wrap([&] {
    dev_trim();
    host_trim();
  });
}

}  // extern "C"
