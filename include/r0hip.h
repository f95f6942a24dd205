/*
 * r0hip — MI355X (gfx950) HAL for risc0-zkp: the C ABI a Rust `HipHal` binds.
 *
 * Drop-in boundary: every entry point below replaces one `extern "C"` symbol the
 * reference's CUDA HAL binds (risc0/zkp/src/hal/cuda.rs -> risc0/sys) or one piece
 * of the `cust` driver crate that cannot run on ROCm. Conventions, mirroring
 * risc0/sys/src/lib.rs:53-75 and SURVEY.md §8(b):
 *   - return NULL on success, else a malloc'd message the caller frees with free()
 *     (the reference's ffi_wrap contract); r0hip_free_error() is provided too;
 *   - pointers are device pointers to raw Montgomery u32 words unless named h_*;
 *     FpExt = 4 consecutive words (AoS), digests = 8 words, matrices column-major;
 *   - sizes/counts are 64-bit element counts (the CUDA ABI's u32 overflows at po2=24);
 *   - every call is complete when it returns (cuda.h:77-100 semantics): results are
 *     visible to the next call and to D2H copies. Work is queued on one HIP stream
 *     per host thread; r0hip_prove_segment runs whole proofs without per-op syncs.
 *   - a thread may opt into deferred completion (r0hip_set_deferred below), the CUDA HAL's
 *     stream-ordered behaviour. Each prototype carries its kind: [queues] = device-only, returns
 *     with its work queued on the thread's stream while the mode is on; [drains] = hands data or
 *     a verdict to the host, always complete on return; [host-only] = no device work. With the
 *     mode off (the default) every [queues] call drains as well.
 * Suites: R0HIP_POSEIDON2 = 0, R0HIP_SHA256 = 1, R0HIP_POSEIDON254 = 2 (zkp/src/core/hash/mod.rs:90-100;
 * the CUDA HAL's CudaHashPoseidon254, zkp/src/hal/cuda.rs:179-233).
 */
#ifndef R0HIP_H
#define R0HIP_H
#include <stddef.h>
#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R0HIP_POSEIDON2 0
#define R0HIP_SHA256 1
#define R0HIP_POSEIDON254 2

/* ---- device / memory (replaces the `cust` crate; zkp/src/hal/cuda.rs:235-381,397-421) ---- */
/* [drains] */
const char* r0hip_init(int device_ordinal);                       /* sppark_init (sys/src/cuda.rs:20) */
/* [drains] */
const char* r0hip_device_info(char* name, size_t name_cap, uint64_t* total_mem);
/* [queues] */
const char* r0hip_alloc(void** d_ptr, size_t bytes);
/* [queues] */
const char* r0hip_free(void* d_ptr);
/* [queues] */
const char* r0hip_memset32(void* d_dst, uint32_t value, size_t count); /* alloc_elem_init (hal/mod.rs:72-83) */
/* [drains] */
const char* r0hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
/* [drains] */
const char* r0hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
/* [queues] */
const char* r0hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
/* page-locked host memory for full-rate witness uploads (cust's LockedBuffer role) */
/* [drains] */
const char* r0hip_host_alloc(void** h_ptr, size_t bytes);
/* [drains] */
const char* r0hip_host_free(void* h_ptr);
/* [drains] */
const char* r0hip_synchronize(void);
/* Completion mode of the calling host thread (thread-local, like the stream; 0 on every new
 * thread, and the library's own pipeline and worker threads never change it). on != 0: the
 * [queues] entry points return after enqueueing, in call order on the thread's stream; results
 * are visible to the thread's later calls and to the host after any [drains] call. *was (may be
 * NULL) receives the previous mode. Turning the mode off drains the thread's stream first and
 * returns an asynchronous error of the queued work, if any. Rules while the mode is on:
 *   - host arrays (h_*) passed to a [queues] call are consumed before it returns;
 *   - a host-side validation failure is returned by the failing call itself, which drains, and
 *     the mode stays on; an asynchronous HIP error is returned by the next [drains] call;
 *   - a buffer may be freed by this thread at any time (its block is reused in stream order),
 *     but only after the work that OTHER threads queued on it has been synchronised there;
 *   - before the thread exits it calls r0hip_synchronize or r0hip_set_deferred(0, ..): a thread
 *     that exits with work queued leaks its device blocks, stream and staging arena. */
/* [host-only] */
const char* r0hip_set_deferred(int on, int* was);
/* Streams one proof of the calling host thread may use (thread-local, like the completion mode;
 * 1 on every new thread, and the library's own pipeline, worker and verifier threads never
 * change it). n = 1 is the single-stream launch sequence. With n >= 2 the code group's
 * commitment (its NTTs, row hashes and tree layers) runs on a side stream: beside the witness
 * generation in r0hip_prove_recursion and r0hip_prove_recursion_keyed, beside the data group's
 * commitment in r0hip_prove_segment, _accum, _trace and _trace_resident. The roots enter the
 * transcript in the same order and the seal is word for word that of n = 1. n is 1..3 (the
 * thread's main stream and two side streams; with the process-wide copy stream these are the 4
 * hardware queues HIP opens by default, no environment variable is needed; only one side stream
 * has work today); any other n is an error that leaves the setting unchanged. *was (may be
 * NULL) receives the previous value. The mode is for a caller that proves one task at a time
 * (an r0vm GPU worker sees one proof's latency): alone, a proof leaves parts of the chip idle
 * that a second stream can fill. r0hip_prove_segments, r0hip_prove_trace_segments and the
 * worker already fill them with other segments and prove at n = 1 whatever the caller's
 * setting. It costs no memory. Every call has joined its side streams when it returns, so the
 * completion rules above are unchanged; the per-op calls are single ops and do not change.
 * While r0hip_set_kernel_timing is on the thread behaves as n = 1. */
/* [drains] */
const char* r0hip_set_proof_streams(uint32_t n, uint32_t* was);
/* Constraint check of the witness inside the provers (thread-local, like the two modes above;
 * off on every new thread, and the library's own pipeline threads never turn it on; a worker's
 * prover threads follow r0hip_worker_set_witness_check). on != 0: every proof of the calling
 * thread that goes through the segment prover (r0hip_prove_segment, _accum, _trace, _trace_backs,
 * _trace_resident and the four r0hip_prove_recursion* calls) evaluates the circuit's constraint
 * polynomial on the 2^po2 rows of its three groups once they are in their final form (after the
 * accumulation, before the accum group is committed), as r0hip_constraint_rows does, with a
 * poly_mix from getrandom(2). Nothing is drawn from the transcript: a witness that satisfies the
 * constraints gives the seal of the mode off, word for word. One that does not fails the call
 * with exactly
 *   constraint check failed: K of N rows, first at cycle R (term T)
 * (K bad rows of N = 2^po2, R the first, T the id in <circuit>.poly.ir of the first violated term,
 * r0hip_constraint_term) and writes no seal, instead of paying for a proof that the receipt check
 * then rejects. r0hip_last_profile carries a check_witness mark while the mode is on. A
 * diagnostic for bring-up, not part of soundness. *was (may be NULL) receives
 * the previous mode. */
/* [host-only] */
const char* r0hip_set_witness_check(int on, int* was);
/* The calling thread's entry-point calls so far, no device work: out[0] = [queues] and [drains]
 * calls made, out[1] = those that drained the stream before returning, out[2] = those that
 * returned with their work only queued. */
/* [host-only] */
const char* r0hip_call_stats(uint64_t out[3]);
void r0hip_free_error(const char* err);
/* A device-to-host copy that runs beside the caller's later calls, for a HAL's host mirrors
 * (hal_hip.rs: a Merkle node heap, read node by node by MerkleTreeProver::prove, merkle.rs:
 * 108-140). The copy goes on a process-wide copy stream; d_src is read as the caller's earlier
 * calls left it (in deferred mode the copy stream waits for the calls still queued), and must
 * not be written or freed until the copy finished. *h_copy = a handle for r0hip_copy_finish, or NULL when the copy is already
 * done (bytes == 0, or h_dst is not r0hip_host_alloc memory: then it is copied before return).
 * r0hip_copy_finish: *done = 1 when the bytes are in h_dst (the handle is then released; a
 * NULL handle is done), 0 if not yet (only with block == 0). */
/* [queues] */
const char* r0hip_memcpy_d2h_start(void* h_dst, const void* d_src, size_t bytes, void** h_copy);
/* [host-only] */
const char* r0hip_copy_finish(void* h_copy, int block, int* done);

/* ---- NTT family (sppark_batch_* in sys/src/cuda.rs:22-46; CPU semantics cpu.rs:305-408) ----
 * Inputs must be canonical field words (< p), as every buffer the Hal hands over is: the first
 * butterfly stage skips its unit twiddle (no Montgomery multiply reduces a staged word), so a
 * non-canonical input word is not reduced there. */
/* expand each of `count` polys of 2^(lg_out-expand_bits) bit-reversed coeffs into out (count x 2^lg_out)
 * and evaluate: Hal::batch_expand_into_evaluate_ntt (hal/mod.rs:102-108; cuda.rs:529-570) */
/* [queues] */
const char* r0hip_batch_expand_into_evaluate_ntt(uint32_t* d_out, const uint32_t* d_in, size_t count,
                                                 uint32_t lg_out, uint32_t expand_bits);
/* Hal::batch_interpolate_ntt (hal/mod.rs:110; cuda.rs:572-590 -> sppark_batch_iNTT) */
/* [queues] */
const char* r0hip_batch_interpolate_ntt(uint32_t* d_io, size_t count, uint32_t lg_size);
/* Hal::zk_shift (hal/mod.rs:123; cuda.rs:690-708 -> sppark_batch_zk_shift) */
/* [queues] */
const char* r0hip_zk_shift(uint32_t* d_io, size_t count, uint32_t lg_size);
/* Hal::batch_bit_reverse (risc0_zkp_cuda_batch_bit_reverse, ffi.cu:89-91) */
/* [queues] */
const char* r0hip_batch_bit_reverse(uint32_t* d_io, size_t count, uint32_t lg_size);

/* ---- polynomial ops ---- */
/* risc0_zkp_cuda_batch_evaluate_any (ffi.cu:93-101): out[k] = sum_i coeffs[which[k]][i] * xs[k]^i */
/* [queues] */
const char* r0hip_batch_evaluate_any(uint32_t* d_out, const uint32_t* d_coeffs, size_t poly_count,
                                     uint32_t lg_poly_size, const uint32_t* d_which, const uint32_t* d_xs,
                                     size_t eval_count);
/* risc0_zkp_cuda_mix_poly_coeffs (ffi.cu:79-87); mix_start / mix are host FpExt (4 words) */
/* [queues] */
const char* r0hip_mix_poly_coeffs(uint32_t* d_out, const uint32_t* d_in, const uint32_t* h_combos,
                                  const uint32_t* h_mix_start, const uint32_t* h_mix, size_t input_size,
                                  size_t count);
/* risc0_zkp_cuda_fri_fold (ffi.cu:75-77): out is 4 x count, in is 4 x 16 x count (SoA planes) */
/* [queues] */
const char* r0hip_fri_fold(uint32_t* d_out, const uint32_t* d_in, const uint32_t* h_mix, size_t count);
/* risc0_zkp_cuda_combos_prepare (ffi.cu:125-143); host arrays, CHECK_SIZE = 16 */
/* [queues] */
const char* r0hip_combos_prepare(uint32_t* d_combos, const uint32_t* h_coeff_u, size_t combo_count,
                                 size_t cycles, const uint32_t* h_reg_sizes, const uint32_t* h_reg_combo_ids,
                                 size_t reg_count, const uint32_t* h_mix);
/* supra_poly_divide (sys/src/cuda.rs:74-79): in-place division of a poly of `size` FpExt by (x - z);
 * h_remainder receives the remainder (Hal::combos_divide asserts it is zero, hal/mod.rs:236-257) */
/* [drains] */
const char* r0hip_poly_divide(uint32_t* d_poly, size_t size, uint32_t* h_remainder, const uint32_t* h_z);
/* Hal::combos_divide batched over all combos: chunk i divides combos[i*cycles..] by each z in
 * h_pows[h_begin[i]..h_begin[i+1]); *bad_chunk = first chunk with a nonzero remainder or -1 */
/* [drains] */
const char* r0hip_combos_divide(uint32_t* d_combos, size_t nchunks, const uint32_t* h_pows,
                                const uint32_t* h_begin, size_t cycles, int64_t* bad_chunk);

/* ---- element-wise (ffi.cu:27-73) ---- */
/* [queues] */
const char* r0hip_eltwise_add_elem(uint32_t* d_out, const uint32_t* d_a, const uint32_t* d_b, size_t count);
/* [queues] */
const char* r0hip_eltwise_copy_elem(uint32_t* d_out, const uint32_t* d_in, size_t count);
/* [queues] */
const char* r0hip_eltwise_zeroize_elem(uint32_t* d_io, size_t count);
/* out (4 x count SoA) = sum over to_add of in (to_add x count FpExt) */
/* [queues] */
const char* r0hip_eltwise_sum_extelem(uint32_t* d_out, const uint32_t* d_in, size_t to_add, size_t count);
/* [queues] */
const char* r0hip_eltwise_copy_elem_slice(uint32_t* d_into, const uint32_t* d_from, size_t from_rows,
                                          size_t from_cols, size_t from_offset, size_t from_stride,
                                          size_t into_offset, size_t into_stride);
/* [queues] */
const char* r0hip_gather_sample(uint32_t* d_dst, const uint32_t* d_src, size_t idx, size_t size, size_t stride);
/* gather_sample straight to the host: h_dst[i] = d_src[idx + i*stride], i < size (no CUDA
 * counterpart). For a HAL whose gather_sample destination is read back before the device uses it
 * (MerkleTreeProver::prove's sample, merkle.rs:111-129: gather_sample, then view): one kernel,
 * one copy and one sync instead of a device allocation, gather_sample, view and free. */
/* [drains] */
const char* r0hip_gather_sample_host(uint32_t* h_dst, const uint32_t* d_src, size_t idx, size_t size,
                                     size_t stride);
/* The sibling paths of n Merkle openings straight to the host (no CUDA counterpart), for a HAL
 * that keeps a node heap on the device only: MerkleTreeProver::prove (merkle.rs:108-140) reads
 * one node per level with get_at, and this call fetches all of one opening's nodes, or those of
 * many openings, with one kernel, one copy and one sync. d_nodes is a heap of heap_digests
 * digests (8 words each) with the root at index 1, as r0hip_hash_fold and r0hip_merkle_tree
 * write it. For j = h_idx[i], h_dst[(i*levels + k)*8 ..] receives nodes[j] for k = 0 and
 * nodes[(j >> k) ^ 1] for 1 <= k < levels: the `other_idx` sequence of merkle.rs:131-138 after
 * its first get_at(j). Checked on the host before any device work, the message naming the index:
 * 1 <= j < heap_digests, levels >= 1, and for levels > 1 (j >> (levels-1)) >= 2. Duplicate
 * indices are allowed; n == 0 does nothing. h_dst may be pageable or r0hip_host_alloc memory. */
/* [drains] */
const char* r0hip_merkle_paths_host(uint32_t* h_dst, const uint32_t* d_nodes, size_t heap_digests,
                                    const uint64_t* h_idx, size_t n, size_t levels);
/* CSR scatter (ffi.cu:108-114): index has cycles+1 entries */
/* [queues] */
const char* r0hip_scatter(uint32_t* d_into, const uint32_t* d_index, const uint32_t* d_offsets,
                          const uint32_t* d_values, size_t cycles);
/* [queues] */
const char* r0hip_prefix_products(uint32_t* d_io, size_t count);
/* not a reference symbol: synthetic witness words (uniform canonical BabyBear values from a
 * counter hash of seed and index) for benches and tests at full size */
/* [queues] */
const char* r0hip_fill_uniform(uint32_t* d_out, size_t count, uint64_t seed);
/* not a reference symbol: keyed noise words, the generator of r0hip_prove_recursion_keyed. The
 * ChaCha20 keystream of RFC 8439 section 2.3 (20 rounds, 32-bit block counter starting at 0)
 * under h_key (8 words) and h_nonce (3 words), both as the RFC's little-endian state words.
 * Element i is the 128-bit little-endian integer made of keystream words 4i..4i+3, reduced
 * mod p = 15 * 2^27 + 1 and stored as the raw word (bias below 2^-96), so block b yields
 * elements 4b..4b+3 and the words do not depend on how the kernel is launched. count <= 2^34.
 * The key is passed to the kernel by value: no device copy of it is made. */
/* [queues] */
const char* r0hip_fill_chacha20(uint32_t* d_out, size_t count, const uint32_t* h_key, const uint32_t* h_nonce);

/* ---- hashing (sppark_poseidon2_{rows,fold}, sppark_poseidon254_{rows,fold}, risc0_zkp_cuda_sha_{rows,fold};
 * sys/src/cuda.rs:49-72) ---- */
/* out[row] = H(matrix[col*rows + row] for col < cols). Poseidon2 / Poseidon254 inputs must be
 * canonical field words (< p): the Poseidon2 full rounds read a word as a signed 32-bit value,
 * which is its value mod p for any word below 2^31 (tests/native/field_equiv.cpp pins
 * [p, 2^31)) but not above. */
/* [queues] */
const char* r0hip_hash_rows(int suite, uint32_t* d_out, const uint32_t* d_matrix, size_t rows, size_t cols);
/* io[output_size + i] = H(io[input_size + 2i], io[input_size + 2i + 1]) (cpu.rs:569-581) */
/* [queues] */
const char* r0hip_hash_fold(int suite, uint32_t* d_io, size_t input_size, size_t output_size);
/* A whole tree in one call: MerkleTreeProver::new's hash_rows into nodes[rows..2rows) and
 * hash_fold of every layer down to the root at nodes[1] (prove/merkle.rs:54-81); d_nodes
 * holds 2*rows digests, rows a power of two. Same words as those calls; the fused form knows
 * each layer's height, so Poseidon2 and SHA-256 layers over all-zero rows store the zero-subtree digests
 * instead of hashing them. */
/* [queues] */
const char* r0hip_merkle_tree(int suite, uint32_t* d_nodes, const uint32_t* d_matrix, size_t rows, size_t cols);

/* ---- circuits (risc0_circuit_{rv32im,recursion}_cuda_eval_check) ---- */
/* circuit: "rv32im" | "recursion". groups[g] = evaluated register group g (accum=0, code=1, data=2),
 * d_check = 4 x 4*2^po2, h_poly_mix = the poly_mix FpExt (powers are expanded on the host) */
/* [drains] */
const char* r0hip_eval_check(const char* circuit, uint32_t* d_check, const uint32_t* const* d_groups,
                             const uint32_t* d_mix, const uint32_t* d_global, const uint32_t* h_poly_mix,
                             uint32_t po2);
/* eval_check and the constraint-rows check first scan the selector columns of the buffers they were
 * given (the generated program's gates) and do not launch a kernel all of whose terms are gated by
 * a column that is zero everywhere: those terms are exactly 0, so the result is word for word the
 * same. R0_EC_SKIP=0 in the environment (read on every call) turns the scan and the skipping off.
 * out[0] = the kernels the calling thread's last such call (a proof's included) launched, out[1]
 * = the kernels its program has; 0, 0 before the first call and for an interpreted circuit. */
/* [host-only] */
const char* r0hip_eval_check_launched(int out[2]);
/* TESTING ONLY: that scan on its own, so a test can reach it. d_matrix holds cols <= 64 columns of `words` words each, one after the
 * other; bit c of *h_mask is set when column c is zero in every word. */
/* [drains] */
const char* r0hip_testing_zero_scan(const uint32_t* d_matrix, size_t cols, size_t words, uint64_t* h_mask);

/* ---- whole segment proof (risc0_zkp::prove::Prover driven as by the circuit's segment prover:
 * circuit/rv32im/src/prove/hal/mod.rs:143-224, circuit/recursion/src/prove/mod.rs:164-230) ----
 * Witness groups are device buffers (column-major, 2^po2 rows); d_global (output_size words) is
 * zeroized in place; h_mix_out (optional) receives the mix values drawn from the transcript.
 * The seal (Vec<u32>) is written to h_seal; *seal_len is its length in words. */
/* [drains] */
const char* r0hip_prove_segment(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                const uint32_t* d_data, const uint32_t* d_accum, uint32_t* d_global,
                                int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                size_t* seal_len, uint32_t* h_mix_out);
/* ---- rv32im BigInt accumulator states (the witness generator's accum injection,
 * circuit/rv32im/src/prove/witgen/mod.rs:178-205) ----
 * One Back::BigInt record of the preflight trace (witgen/preflight.rs:55-56, 471-479), holding
 * the fields of BigIntState (witgen/bigint.rs:36-44) that BigIntAccum::step reads: the cycle
 * (row), poly_op (PolyOp, bigint.rs:62-70: 0 Reset, 1 Shift, 2 SetTerm, 3 AddTotal, 4 Carry1,
 * 5 Carry2, 6 EqZero), coeff (BigIntState::coeff = the instruction's coefficient + 4) and the
 * 16 bytes. Records are passed in trace order (strictly increasing rows). */
typedef struct r0hip_bigint_back {
  uint32_t row;
  uint32_t poly_op;
  uint32_t coeff;
  uint8_t bytes[16];
} r0hip_bigint_back;
/* BigIntAccum::new(final mix) then ::step per record (witgen/byte_poly.rs:381-470): the state
 * after each record, 12 Montgomery words (poly, term, total; BigIntAccumState::as_array) per
 * record into h_states. h_mix is the whole rv32im mix (36 words; the last 4 are the final
 * mix). Fails as the reference does on an EqZero whose goal is nonzero ("Invalid eqz in
 * bigint accum"). Host-only. */
/* [host-only] */
const char* r0hip_rv32im_bigint_accum_states(const uint32_t* h_mix, const r0hip_bigint_back* h_backs, size_t n,
                                             size_t rows, uint32_t* h_states);
/* The same states computed on the device (BigIntAccum::step, byte_poly.rs:381-470, as three
 * parallel scans over the records: poly an affine scan, term a last-writer scan, total a
 * segmented sum; EqZero checked per record): the n records are uploaded as they are and
 * d_states (device memory) receives n x 12 words, in record order, equal to what the host
 * function writes. n <= rows <= 2^26. Fails with the host function's messages, at the earliest
 * record in trace order that fails any check. Always takes the device path; n == 0 is a no-op.
 * Complete on return. */
/* [drains] */
const char* r0hip_rv32im_bigint_accum_states_device(uint32_t* d_states, const uint32_t* h_mix,
                                                    const r0hip_bigint_back* h_backs, size_t n, size_t rows);
/* The states above scattered into accum columns 0..11 (BigIntAccumState::offsets,
 * byte_poly.rs:362-377) of each record's row of d_accum (column-major, `rows` rows): what
 * WitnessGenerator::accum does before step_accum (witgen/mod.rs:187-205). From 4096 records
 * on, the states are computed on the device (as r0hip_rv32im_bigint_accum_states_device) and
 * scattered from device memory; below that the host loop is faster and its states are
 * uploaded. The words and the errors are the same either way. */
/* [queues] */
const char* r0hip_rv32im_bigint_accum_inject(uint32_t* d_accum, size_t rows, const uint32_t* h_mix,
                                             const r0hip_bigint_back* h_backs, size_t n);

/* ---- whole segment proof with the accumulation on the device: the prove_core sequence above,
 * with the circuit's accumulation between the mix draw and the accum commit, as the reference
 * runs it (rv32im: WitnessGenerator::accum, circuit/rv32im/src/prove/witgen/mod.rs:178-221, over
 * risc0_circuit_rv32im_cuda_accum; recursion: prove/witgen.rs:138-177 over
 * risc0_circuit_recursion_cuda_accum). d_accum is the accum group as the witness generator
 * allocated it: every word INVALID (0xFFFFFFFF), plus for recursion the ZK noise rows the caller
 * draws (witgen.rs:143-158). rv32im: h_bigint/n_bigint are the trace's BigInt backs; their
 * accumulator states, computed with the mix this call draws, are injected before the step
 * (r0hip_rv32im_bigint_accum_inject; witgen/mod.rs:182-205). Recursion takes none. The group is
 * accumulated over work_cycles cycles (rv32im: the preflight cycle count, 2^po2; recursion:
 * work_cycles), INVALID words are zeroized, and the group is committed. The other arguments
 * are r0hip_prove_segment's. */
/* [drains] */
const char* r0hip_prove_segment_accum(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                      const uint32_t* d_data, uint32_t* d_accum, size_t work_cycles,
                                      const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* d_global,
                                      int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                      size_t* seal_len, uint32_t* h_mix_out);
/* ---- rv32im witness side: accumulation phases 2-3 (risc0_circuit_rv32im_cuda_accum after its
 * stepAccum kernel, rv32im-sys/kernels/cuda/ffi.cu:480-509; CPU ffi.cpp:326-360): inclusive
 * prefix sums of the last 4 accum columns over rows [0, last_cycle), then every row adds the
 * previous row's prefix values to the machine columns [23, cols - 4). d_accum is the accum
 * group, column-major with `rows` rows, after the per-cycle phase (r0hip_rv32im_accum runs both). */
/* [queues] */
const char* r0hip_rv32im_accum_finalize(uint32_t* d_accum, size_t rows, size_t cols, size_t last_cycle);
/* ---- rv32im witness side: the whole accumulation (risc0_circuit_rv32im_cuda_accum,
 * rv32im-sys/kernels/cuda/ffi.cu:362-514; CPU risc0_circuit_rv32im_cpu_accum, ffi.cpp:313-368):
 * phase 1, the per-cycle accumulation step (stepAccum, ffi.cpp:238-247, generated from the
 * reference's step_TopAccum), for cycles [0, last_cycle), then phases 2-3 as above. d_data is
 * the data group (211 columns), d_accum the accum group (cols = 103) as the prover allocates
 * it (every word INVALID, 0xFFFFFFFF); d_global (90 words) and d_mix (36 words) as in
 * AccumBuffers (witgen.h). Columns are `rows` long. */
/* [queues] */
const char* r0hip_rv32im_accum(const uint32_t* d_data, uint32_t* d_accum, const uint32_t* d_global,
                               const uint32_t* d_mix, size_t rows, size_t cols, size_t last_cycle);

/* ---- rv32im witness generation (risc0_circuit_rv32im_cuda_witgen / _cpu_witgen,
 * rv32im-sys/kernels/cuda/ffi.cu:431-472, kernels/cxx/ffi.cpp:267-308; bound in
 * rv32im-sys/src/lib.rs:55-86 and called from circuit/rv32im/src/prove/hal/cuda.rs:60-101) ----
 * The same three structs the reference passes (RawBuffer, RawExecBuffers, RawPreflightTrace,
 * rv32im-sys/src/lib.rs:20-76), field for field. buffers->global (rows 1, cols 90) and
 * buffers->data (cols 211, rows a power of two) are DEVICE pointers: the global vector as
 * build_global_vec makes it and the data group all INVALID with the injector scattered in
 * (witgen/mod.rs:146-162; r0hip_scatter). preflight's arrays are HOST pointers, as in the
 * reference: `cycles` RawPreflightCycle records (36 bytes), txns RawMemoryTransaction (20
 * bytes), bigint_bytes. step_Top runs for cycles [0, cycles) in the reference's two phases
 * (before and after table_split_cycle). mode (0 parallel, 1 forward, 2 reverse) is checked and
 * every mode runs the parallel schedule, which gives the same words on any trace the
 * reference accepts. Fails as the reference throws: EQZ ("eqz failure at: ..."), a
 * transaction at another cycle or address, reads of unset words, inconsistent re-stores, bad
 * lookups. Zeroize stays the caller's (witgen/mod.rs:166-170). */
typedef struct r0hip_raw_buffer {
  uint32_t* buf;
  size_t rows;
  size_t cols;
  bool checked;
} r0hip_raw_buffer;
typedef struct r0hip_raw_exec_buffers {
  r0hip_raw_buffer global;
  r0hip_raw_buffer data;
} r0hip_raw_exec_buffers;
typedef struct r0hip_raw_preflight_trace {
  const void* cycles;
  const void* txns;
  const uint8_t* bigint_bytes;
  uint32_t txns_len;
  uint32_t bigint_bytes_len;
  uint32_t table_split_cycle;
} r0hip_raw_preflight_trace;
/* [drains] */
const char* r0hip_rv32im_witgen(uint32_t mode, const r0hip_raw_exec_buffers* buffers,
                                const r0hip_raw_preflight_trace* preflight, uint32_t cycles);

/* ---- rv32im prove_core from a preflight trace: SegmentProverImpl::prove_core
 * (circuit/rv32im/src/prove/hal/mod.rs:143-224) over WitnessGenerator::new and ::accum
 * (witgen/mod.rs:106-223), every step on the device ----
 * h_global: build_global_vec's 90 Montgomery words (INVALID where unset, witgen/mod.rs:272-327).
 * The injector (Injector, witgen/mod.rs:329-378) as hal.scatter takes it: h_inj_index
 * (inj_rows + 1 entries), h_inj_offsets / h_inj_values (h_inj_index[inj_rows] entries:
 * col * 2^po2 + row, Montgomery value). preflight as r0hip_rv32im_witgen takes it (cycles =
 * 2^po2 records); mode as there. h_bigint / n_bigint: the trace's Back::BigInt records, as
 * r0hip_prove_segment_accum takes them. Runs: data INVALID, scatter, stepExec (both phases),
 * zeroize, then the prove_core sequence with the version word 2 (RV32IM_SEAL_VERSION) and the
 * accumulation on the device. Seal and mix out as r0hip_prove_segment. */
/* Host arrays of 64 KiB or more that lie inside r0hip_host_alloc blocks are copied to the
 * device directly; others are staged through the calling thread's page-locked arena. */
/* [drains] */
const char* r0hip_prove_segment_trace(int suite, uint32_t po2, uint32_t mode, const uint32_t* h_global,
                                      const uint32_t* h_inj_index, size_t inj_rows, const uint32_t* h_inj_offsets,
                                      const uint32_t* h_inj_values, const r0hip_raw_preflight_trace* preflight,
                                      const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* h_seal,
                                      size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out);

/* ---- the injector in its compact form: the preflight's Back records ----
 * build_injector (circuit/rv32im/src/prove/witgen/mod.rs:226-270) expands, row by row, the row's
 * Back (witgen/preflight.rs:47-57) and Injector::set_cycle (mod.rs:353-365) into the (offset,
 * value) list hal.scatter takes. Here the caller hands over what the expansion reads,
 * trace.backs and trace.cycles, and the expansion runs on the device. One record per row whose
 * Back is not None; its payload is the reference's own array, PLAIN u32 words: the device does
 * what Injector::set does, Val::from(u32) = encode(x % P) (core/src/field/baby_bear.rs:202-204).
 * The payload's word k goes to column k of the kind's column list (Poseidon2State::offsets,
 * Sha2State::fp_offsets, BigIntState::offsets; ECALL_S0..S2); a SHA-2 record's last three words
 * (a, e, w; Sha2State::u32_array) go out as Injector::set_u32_bits writes them, bit i of word k
 * in column u32_offsets[k] + i. */
#define R0HIP_BACK_ECALL     1  /*  3 words: s0, s1, s2                      (mod.rs:240-247) */
#define R0HIP_BACK_POSEIDON2 2  /* 39 words: Poseidon2State::as_array        (witgen/poseidon2.rs:136-179) */
#define R0HIP_BACK_SHA2      3  /* 10 words: Sha2State::fp_array (7), a, e, w (witgen/sha2.rs:45-59) */
#define R0HIP_BACK_BIGINT    4  /* 22 words: BigIntState::as_array           (witgen/bigint.rs:213-238) */
typedef struct r0hip_back { uint32_t row; uint32_t kind; uint32_t word; } r0hip_back; /* word: index of the payload's first word */
typedef struct r0hip_backs {
  const r0hip_back* recs; size_t n;        /* rows strictly increasing; Back::None rows have no record */
  const uint32_t* words;  size_t n_words;  /* payloads, PLAIN u32 as the reference's arrays hold them */
  size_t inj_rows;                         /* rows that get the set_cycle columns (trace.cycles.len()), <= 2^po2 */
} r0hip_backs;
/* build_injector plus hal.scatter in front of r0hip_rv32im_witgen: writes into d_data (211
 * columns x rows, column-major, every word INVALID or as r0hip_prove_segment_trace's fill leaves
 * it) the words the scatter of build_injector's output writes: for every row r < inj_rows the
 * five set_cycle columns from r and h_cycles[r].{pc, state, machine_mode} (h_cycles: inj_rows
 * RawPreflightCycle records, host), and every record's payload in its kind's columns. No other
 * word is touched. The struct and its arrays are on the host and are consumed before the call
 * returns. Checked on the host before any launch, in O(n), the message naming the record: recs /
 * words NULL with a nonzero count, rows not strictly increasing or >= inj_rows, inj_rows > rows,
 * a kind outside 1..4, a payload that ends past n_words. */
/* [queues] */
const char* r0hip_rv32im_inject_backs(uint32_t* d_data, size_t rows, const void* h_cycles, const r0hip_backs* backs);
/* r0hip_prove_segment_trace from the Back records: the same sequence and the same seal, with the
 * injector expanded on the device from `backs` (checked as above, against 2^po2 rows) and the
 * accumulation's r0hip_bigint_back records derived on the host from the BigInt payloads (row,
 * poly_op = word 3, coeff = word 4, bytes = the low 8 bits of words 5..20), in O(n). A record
 * whose kind's columns are not ones its row's instruction arm takes from the injector is handled
 * as the same entries of a CSR injector are: the outcome, a seal or the reference's error text,
 * is that of r0hip_prove_segment_trace on the expanded list. */
/* [drains] */
const char* r0hip_prove_segment_trace_backs(int suite, uint32_t po2, uint32_t mode, const uint32_t* h_global,
                                            const r0hip_raw_preflight_trace* preflight, const r0hip_backs* backs,
                                            uint32_t* h_seal, size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out);

/* The same with every input already resident in device memory (the global vector, the
 * injector arrays, and d_preflight's cycles / txns / bigint_bytes are DEVICE pointers; the
 * struct itself and h_bigint are on the host): what the benchmark times, inputs in HBM.
 * Injector offsets outside the data group are skipped. */
/* [drains] */
const char* r0hip_prove_segment_trace_resident(int suite, uint32_t po2, uint32_t mode, const uint32_t* d_global,
                                               const uint32_t* d_inj_index, size_t inj_rows,
                                               const uint32_t* d_inj_offsets, const uint32_t* d_inj_values,
                                               const r0hip_raw_preflight_trace* d_preflight,
                                               const r0hip_bigint_back* h_bigint, size_t n_bigint, uint32_t* h_seal,
                                               size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out);

/* ---- recursion witness side: the accumulation step (risc0_circuit_recursion_cuda_accum,
 * recursion-sys/kernels/cuda/ffi.cu; CPU driver recursion-sys/kernels/cxx/ffi.cpp:160-217,
 * called from circuit/recursion/src/prove/witgen.rs:162-170): for cycles [0, work_cycles) the
 * per-cycle accumulator factors (step_compute_accum), their inclusive prefix product, and the
 * accum-group registers (step_verify_accum) written into d_accum. Groups are column-major with
 * total_cycles rows (a power of two); d_mix holds the mix values, d_global the globals. Cells
 * no step writes are left as they were (the reference leaves them INVALID for the caller to
 * zeroize, witgen.rs:172-175). */
/* [queues] */
const char* r0hip_recursion_accum(const uint32_t* d_ctrl, const uint32_t* d_global, const uint32_t* d_data,
                                  const uint32_t* d_mix, uint32_t* d_accum, size_t work_cycles,
                                  size_t total_cycles);

/* ---- recursion witness generation (risc0_circuit_recursion_cuda_witgen / _cpu_witgen,
 * recursion-sys/kernels/cxx/ffi.cpp:191-205, driven by circuit/recursion/src/prove/witgen.rs:
 * 91-100 in StepMode::Parallel) ----
 * From the control group (d_ctrl, 23 columns x total_cycles rows, the program's rows first)
 * and the preflight trace (RawPreflightTrace, prove/preflight.rs): h_wom the write-once
 * memory (n_wom FpExt, 4 Montgomery words each), h_cycles {iopIdx, isParSafe} per work
 * cycle (n_cycles pairs of words), h_iops the IOP values read (n_iops FpExt). Fills d_data
 * (128 columns x total_cycles, INVALID-filled by the caller as witgen.rs:68-72 allocates it)
 * and d_global (32 words, INVALID-filled): step_exec per cycle (runs of non-parallel-safe
 * cycles in order), the WOM argument sorted and scanned, injectWomBacks, step_verify_mem.
 * Fails with the reference's message on a failed check ("eqz failed at: ..."). ZK noise and
 * zeroize stay the caller's (witgen.rs:101-123). */
/* [drains] */
const char* r0hip_recursion_witgen(const uint32_t* d_ctrl, uint32_t* d_data, uint32_t* d_global, size_t total_cycles,
                                   const uint32_t* h_wom, size_t n_wom, const uint32_t* h_cycles, size_t n_cycles,
                                   const uint32_t* h_iops, size_t n_iops);
/* A whole recursion proof from a program and its preflight (RecursionProverImpl::prove,
 * circuit/recursion/src/prove/mod.rs:160-230): witness generation as above, ZK noise in the
 * last 1024 rows of data and accum (per-cell values of r0hip_fill_uniform(noise_seed) and
 * (noise_seed + 1), laid out as witgen.rs:101-158 copies its noise matrices), zeroize, then
 * r0hip_prove_segment_accum's sequence with work cycles = n_cycles. po2 >= 11 and n_cycles <=
 * 2^po2 - 1024 (program.rs:57). Seal and mix out as r0hip_prove_segment.
 * DETERMINISTIC, for tests and benches: the noise is a counter hash of the 64-bit noise_seed,
 * not a random draw, so a seal made by this call is not zero-knowledge. The call to ship is
 * r0hip_prove_recursion_keyed below. */
/* [drains] */
const char* r0hip_prove_recursion(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom, size_t n_wom,
                                  const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops, size_t n_iops,
                                  uint64_t noise_seed, uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                  uint32_t* h_mix_out);
/* The same sequence with the ZK noise drawn from a keyed ChaCha20 stream on the device
 * (r0hip_fill_chacha20), as the reference draws it from its OS-seeded CSPRNG (circuit/recursion/
 * src/prove/witgen.rs:103-105, 146-149). The data noise matrix is the stream of h_key with nonce
 * {0, lo32(stream_id), hi32(stream_id)}, the accum noise matrix the one with nonce {1, lo32,
 * hi32}; element i of a stream is word i of the cols x 1024 noise buffer, where
 * r0hip_prove_recursion puts word i of its generator. h_key: 8 words, or NULL for 32 bytes of
 * getrandom(2) drawn for this call (the call fails if the OS gives none; there is no weaker
 * source). A caller's key must never meet the same stream_id twice. Host copies of the key are
 * wiped when the call returns. */
/* [drains] */
const char* r0hip_prove_recursion_keyed(int suite, uint32_t po2, const uint32_t* d_ctrl, const uint32_t* h_wom,
                                        size_t n_wom, const uint32_t* h_cycles, size_t n_cycles,
                                        const uint32_t* h_iops, size_t n_iops, const uint32_t* h_key,
                                        uint64_t stream_id, uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                        uint32_t* h_mix_out);

/* ---- resident recursion programs (circuit/recursion/src/prove/program.rs:33-104; the control
 * group of WitnessGenerator::new, prove/witgen.rs:57-67; its commitment, zkp/src/prove/prover.rs:
 * 81-108) ----
 * r0vm proves a handful of fixed programs (lift, join, resolve, ...) thousands of times, and the
 * control group and its commitment depend only on (program, po2, suite). A handle makes both
 * once; every proof from it skips the host transposition, the 23 x 2^po2 word upload and the
 * control group's NTTs, row hashes and Merkle tree. */
typedef struct r0hip_recursion_program r0hip_recursion_program;
#define R0HIP_CODE_ENCODED    0  /* plain u32 words as a .zkr holds them; Elem::from per word (program.rs:50-58) */
#define R0HIP_CODE_MONTGOMERY 1  /* Program.code as the Rust side holds it: canonical Montgomery words */
/* Program::from_encoded + WitnessGenerator::new's control group + Program::compute_control_id
 * (program.rs:46-104, witgen.rs:57-67). h_code: n_words = 23 * code_rows words, row-major, 23
 * per program row (Program.code and the .zkr stream), in the given form. On the device the rows
 * become the control group (column-major, 2^po2 rows, rows from code_rows on zero), which is
 * committed as every proof commits it (interpolate + zk shift, 4x evaluate, row hashes, Merkle
 * tree). The handle keeps the group, its coefficients, evaluations and node heap in four
 * dedicated allocations (not pool blocks; counted by r0hip_mem_stats, live and reserved) that
 * nothing writes after this call, plus a host copy of the root: the control id. Complete on
 * return: any stream of any thread may read the handle. Refused on the host, before any device
 * call, with the argument (and for a word its index) in the message: a NULL out or h_code, an
 * unknown suite or form, po2 outside 11..24, n_words 0 or not a multiple of 23, more than
 * 2^po2 - 1024 rows (program.rs:56-57), and in the Montgomery form a word >= p. In the encoded
 * form every u32 is legal (Elem::from reduces it). */
/* [drains] */
const char* r0hip_recursion_program_create(r0hip_recursion_program** out, int suite, uint32_t po2,
                                           const uint32_t* h_code, size_t n_words, int form);
/* What a handle holds; every out pointer may be NULL. control_id: the control group's Merkle
 * root (program.rs:74-104), the digest r0hip_verify_seal reports as the code root of a seal
 * made from this program. device_bytes: the four allocations, 4 * (23 + 23 + 92) * 2^po2 for the
 * group, coefficients and evaluations plus 64 * 4 * 2^po2 for the node heap. */
/* [host-only] */
const char* r0hip_recursion_program_info(const r0hip_recursion_program* program, int* suite, uint32_t* po2,
                                         size_t* code_rows, uint32_t control_id[8], uint64_t* device_bytes);
/* The handle's control group on the device (23 columns x 2^po2 words), read-only, valid until
 * r0hip_recursion_program_destroy: what r0hip_recursion_witgen, r0hip_recursion_accum and
 * r0hip_prove_recursion_keyed take as d_ctrl. */
/* [host-only] */
const char* r0hip_recursion_program_ctrl(const r0hip_recursion_program* program, const uint32_t** d_ctrl);
/* RecursionProverImpl::prove (circuit/recursion/src/prove/mod.rs:160-230) from a handle:
 * r0hip_prove_recursion_keyed's sequence (witness generation from the handle's control group,
 * keyed ChaCha20 noise, zeroize, data commit, mix, accumulation, accum commit, finalize) with
 * the control group's commitment taken from the handle; its root enters the transcript where
 * the commit would put it. Seal and mix are word for word those of r0hip_prove_recursion_keyed
 * on the same control group, key and stream_id. n_cycles must equal the handle's code_rows
 * (witgen.rs:80). No code commit is left to move to a side stream: with r0hip_set_proof_streams
 * >= 2 the call runs as at n = 1. Any number of threads may prove from one handle at once; each
 * proof holds a use count until it returns. */
/* [drains] */
const char* r0hip_prove_recursion_program(const r0hip_recursion_program* program, const uint32_t* h_wom, size_t n_wom,
                                          const uint32_t* h_cycles, size_t n_cycles, const uint32_t* h_iops,
                                          size_t n_iops, const uint32_t* h_key, uint64_t stream_id, uint32_t* h_seal,
                                          size_t seal_cap, size_t* seal_len, uint32_t* h_mix_out);
/* ---- recursion proofs from a program and its input words (RecursionProver::prove(program,
 * input), circuit/recursion/src/prove/mod.rs:165; the preflight, prove/preflight.rs:181-627) ----
 * The entry points above take the preflight's arrays. These take what the reference calls
 * `input` and run the preflight themselves, natively on the host (csrc/recursion_preflight.h).
 * Covered: the micro ops CONST .. EXTRACT, the macro ops nop, wom_init, wom_fini, set_global,
 * bit_and_elem, bit_op_shorts, sha_init, sha_load, sha_mix and sha_fini, and the four Poseidon2
 * row kinds. Refused when the program is decoded, naming the row: checked_bytes rows (no C++
 * witness generator runs them). A run fails with the reference's message where it has one, followed by
 * " (cycle N)": "Equality check failed: Expecting [..] == [..]", "WOM A overwritten with [..]
 * from [..]" (a cell rewritten with the same value is legal), "Illegal recursion op", "Unknown
 * opcode"; where the reference panics, with the library's own: "input exhausted: ...",
 * "READ_IOP_BODY on an empty IOP body", "READ_IOP_HEADER while the IOP body has K unread
 * values", "WOM read of address A past the memory's N cells". The library's limit: a WOM address
 * at or above 16 * 2^po2 cells is refused (the reference grows its memory to any address below
 * p); the witness generator allows 9 WOM argument rows per cycle, so a program it accepts stays
 * below.
 *
 * r0hip_recursion_preflight: the preflight alone, from the program's words (h_code, n_words,
 * form and po2 as r0hip_recursion_program_create takes them; no handle, so no device is
 * needed). Size query: with all four out arrays NULL only the counts are written, and they
 * depend on the program alone (every write address, READ_IOP_BODY and output position is in the
 * code). Otherwise all four arrays are given with their capacities (h_wom and h_iops in cells of
 * 4 words, h_cycles in cycles of 2 words {iop_idx, is_par_safe}, h_output in words) and are
 * filled as r0hip_recursion_witgen takes them: WOM and IOP values as Montgomery words, the
 * output (Preflight.output) as plain integers. On a run-time failure h_cycles is complete and
 * the other arrays hold what the run wrote before it stopped. */
/* [host-only] */
const char* r0hip_recursion_preflight(const uint32_t* h_code, size_t n_words, int form, uint32_t po2,
                                      const uint32_t* h_input, size_t n_input, uint32_t* h_wom, size_t wom_cap,
                                      size_t* n_wom, uint32_t* h_cycles, size_t cycles_cap, size_t* n_cycles,
                                      uint32_t* h_iops, size_t iops_cap, size_t* n_iops, uint32_t* h_output,
                                      size_t output_cap, size_t* n_output);
/* Makes what every proof from input shares, once per handle: on the host the decoded op table
 * with each cycle's {iop_idx, is_par_safe}; on the device, in one dedicated allocation, the
 * witness generator's plan (the exec runs, each cycle's first IOP value, the runs ordered by
 * bucket; the bucket counts stay on the host). Idempotent and thread-safe; the from-input entry
 * points call it themselves. r0hip_recursion_program_info and its device_bytes do not change;
 * r0hip_recursion_program_input_info reports the plan. Freed by r0hip_recursion_program_destroy. */
/* [drains] */
const char* r0hip_recursion_program_prepare_input(const r0hip_recursion_program* program);
typedef struct r0hip_recursion_input_info {
  uint32_t prepared;           /* 0: not prepared yet, every other field 0 */
  uint32_t n_runs;             /* exec runs (MachineContext::parStepExec) */
  uint32_t bucket_runs[9];     /* runs per specialised exec launch */
  size_t n_wom;                /* WOM cells of a complete run */
  size_t n_iops;               /* IOP values */
  size_t n_output;             /* output words */
  uint64_t n_input;            /* input words the READ_IOP_HEADER ops consume */
  uint64_t plan_device_bytes;  /* the plan's dedicated allocation */
  uint64_t plan_host_bytes;    /* op table and cycle table */
} r0hip_recursion_input_info;
/* [host-only] */
const char* r0hip_recursion_program_input_info(const r0hip_recursion_program* program,
                                               r0hip_recursion_input_info* out);
/* RecursionProver::prove(program, input) from a handle: the preflight on the calling thread
 * (written straight into page-locked staging while the group fills run), witness generation
 * from the handle's plan (no run keys, no run sort, no host synchronisation before the final
 * error read; only the WOM and the IOP values are copied up), then r0hip_prove_recursion_program's
 * sequence. Seal and mix are word for word those of r0hip_prove_recursion_program on the
 * preflight's arrays with the same key and stream_id. h_output (optional, output_cap words)
 * receives Preflight.output; n_output (optional) its length, written before a too-small buffer
 * is refused. A preflight failure is returned as the error. */
/* [drains] */
const char* r0hip_prove_recursion_program_input(const r0hip_recursion_program* program, const uint32_t* h_input,
                                                size_t n_input, const uint32_t* h_key, uint64_t stream_id,
                                                uint32_t* h_seal, size_t seal_cap, size_t* seal_len,
                                                uint32_t* h_mix_out, uint32_t* h_output, size_t output_cap,
                                                size_t* n_output);
/* Host milliseconds of the preflight inside the calling thread's last
 * r0hip_prove_recursion_program_input (0 before the first): a thread's figure, like
 * r0hip_last_profile, for benchmarks that report the call less its preflight. */
/* [host-only] */
const char* r0hip_recursion_last_preflight_ms(double* out);
/* Frees the handle and its device memory (after it and r0hip_trim, r0hip_mem_stats' live bytes
 * are what they were before create). While a proof runs from the handle or a worker job that
 * names it has not been handed back, it returns an error and frees nothing. */
/* [drains] */
const char* r0hip_recursion_program_destroy(r0hip_recursion_program* program);

/* ---- segment pipeline (r0vm's per-GPU worker queue, r0vm/src/actors/worker.rs:75-76, over the
 * zkvm's per-segment prove loop, zkvm/src/host/server/prove/prover_impl.rs:84-94) ----
 * Proves njobs segments of one (circuit, suite, po2) from HOST witness groups: an uploader thread
 * copies each job's groups into one of in_flight+1 device buffer sets, in 48-column chunks, while
 * in_flight provers (in_flight - 1 threads and the calling thread) prove on their own streams; a
 * prover starts a job at once and commits each group chunk by chunk as it lands (Poseidon2 and
 * SHA-256; Poseidon254 waits for whole groups). Host buffers must stay valid until the call
 * returns and should be page-locked (r0hip_host_alloc) for full PCIe rate. Per job: seal into
 * h_seal (seal_cap words), its length in seal_len, mix values into h_mix_out (optional), and
 * error = NULL or a malloc'd message (free() it). Returns NULL when every job succeeded. Seals
 * equal r0hip_prove_segment's. (Round 5 appended a `trace` pointer to this struct; trace jobs
 * now have their own entry point below and this struct has its round-4 layout again.) */
typedef struct r0hip_segment_job {
  const uint32_t* h_code;
  const uint32_t* h_data;
  const uint32_t* h_accum;  /* rv32im: NULL = accumulate on the device (as r0hip_prove_segment_accum,
                               work cycles 2^po2); the group then never crosses PCIe */
  const uint32_t* h_global; /* output_size words; zeroized on the device copy only */
  const r0hip_bigint_back* h_bigint; /* device accumulation only: the trace's BigInt backs, as */
  size_t n_bigint;                   /* r0hip_prove_segment_accum takes them (NULL, 0 if none) */
  uint32_t* h_seal;
  size_t seal_cap;
  size_t seal_len;
  uint32_t* h_mix_out;
  const char* error;
} r0hip_segment_job;
/* [drains] */
const char* r0hip_prove_segments(const char* circuit, int suite, uint32_t po2, int write_version, uint32_t version,
                                 r0hip_segment_job* jobs, size_t njobs, uint32_t in_flight);

/* ---- the GPU worker unit from preflight traces: rv32im SegmentProverImpl::prove_core
 * (circuit/rv32im/src/prove/hal/mod.rs:143-224) per job, as r0vm's GPU worker runs it from the
 * executor's segments (r0vm/src/actors/worker.rs:186-260, job/proof.rs:238-323), with the CUDA
 * prove_core's trace upload (circuit/rv32im/src/prove/witgen/mod.rs:135-176) done by an uploader
 * thread: the trace, the injector and the global vector go into one of in_flight+1 device trace
 * sets while in_flight provers (in_flight - 1 threads and the calling thread) run witness
 * generation, accumulation and the proof from the others. The injector is checked on the host as
 * r0hip_prove_segment_trace checks it. Seals equal r0hip_prove_segment_trace's (version word 2).
 * verify != 0: every seal is checked by r0hip_verify_seal (the validity equation included) on a
 * host thread while the GPU proves the next jobs, as ProverImpl::prove_segment_core verifies a
 * receipt before returning it (zkvm/src/host/server/prove/prover_impl.rs:262-280); a seal that
 * fails sets that job's error ("receipt verification failed: ...") and the other jobs still
 * return. verify == R0HIP_VERIFY_RECEIPTS_DEVICE (2), here and in r0hip_worker_create: the same
 * check through r0hip_verify_seal_on(R0HIP_VERIFY_DEVICE, ...), the seal's Merkle openings hashed
 * on the verifier thread's own stream; every other nonzero value is the host check.
 * Host arrays must stay valid until the call returns. */
#define R0HIP_VERIFY_RECEIPTS_DEVICE 2
typedef struct r0hip_trace_input {
  uint32_t mode;                      /* as r0hip_rv32im_witgen */
  const uint32_t* h_global;           /* build_global_vec's 90 Montgomery words */
  const uint32_t* h_inj_index;        /* inj_rows + 1 entries */
  size_t inj_rows;
  const uint32_t* h_inj_offsets;      /* h_inj_index[inj_rows] entries each */
  const uint32_t* h_inj_values;
  r0hip_raw_preflight_trace preflight; /* host pointers; 2^po2 cycle records */
} r0hip_trace_input;
typedef struct r0hip_trace_job {
  r0hip_trace_input trace;
  const r0hip_bigint_back* h_bigint;  /* the trace's BigInt backs (NULL, 0 if none) */
  size_t n_bigint;
  uint32_t* h_seal;                   /* out: the seal (seal_cap words), its length in seal_len */
  size_t seal_cap;
  size_t seal_len;
  uint32_t* h_mix_out;                /* out (optional): the 36 mix words */
  const char* error;                  /* out: NULL or a malloc'd message (free() it) */
  int verified;                       /* out: 1 when the seal passed r0hip_verify_seal */
  double verify_ms;                   /* out: host milliseconds of that check */
  double prove_ms;                    /* out: host milliseconds from a prover taking the job to its
                                         seal in host memory (the wait for its upload included) */
} r0hip_trace_job;
/* [drains] */
const char* r0hip_prove_trace_segments(int suite, uint32_t po2, r0hip_trace_job* jobs, size_t njobs,
                                       uint32_t in_flight, int verify);

/* ---- the GPU worker: a persistent queue of mixed jobs (r0vm's GPU actor, r0vm/src/actors/
 * worker.rs:165, 289-312: tasks arrive one at a time, ProveSegmentCore interleaved with Lift and
 * Join) ----
 * r0hip_worker_create starts an uploader thread, in_flight prover threads and, with verify != 0,
 * a verifier thread, each with its own stream, pool and staging, and allocates in_flight + 1
 * device sets sized for max_po2 (2..24). The calling thread proves nothing. With in_flight <= 3
 * the uploader and the provers fit the 4 hardware queues HIP opens by default. h_noise_key: the
 * 8-word ChaCha20 key of the recursion jobs' ZK noise; NULL draws 32 bytes of getrandom(2) for
 * the worker's lifetime (create fails if the OS gives none). A caller's key makes runs
 * reproducible and is FOR TESTS ONLY: a key reused across workers repeats nonces.
 * r0hip_worker_submit checks what needs no device (the kind, the suite, po2 <= max_po2, for a
 * recursion job po2 >= 11 and n_cycles <= 2^po2 - 1024, null pointers); a failure returns an
 * error and queues nothing. Otherwise it clears the job's out fields, assigns job->ticket (the
 * submission number, from 0), appends the job to a FIFO and returns without touching the GPU.
 * Jobs start in ticket order. The job struct and every host array it names must stay valid
 * until r0hip_worker_wait hands the job back.
 * Per job: rv32im jobs (kind R0HIP_JOB_RV32IM_TRACE) are staged and proved as
 * r0hip_prove_trace_segments proves them, at the job's own po2; their seals equal
 * r0hip_prove_segment_trace's. Recursion jobs (R0HIP_JOB_RECURSION) take the control group from
 * host memory (staged by the uploader) and are proved as r0hip_prove_recursion_keyed proves
 * them with the worker's key and stream_id = the job's ticket, so the seal equals that call's on
 * the same inputs. A job's own failure goes to job->error (malloc'd, free() it) and the other
 * jobs continue. Jobs of kind R0HIP_JOB_RV32IM_BACKS are rv32im jobs whose injector is job->backs
 * (r0hip_backs above) instead of the CSR arrays: they use trace.mode, trace.h_global and
 * trace.preflight, ignore trace.h_inj_* / inj_rows and h_bigint / n_bigint (the BigInt records
 * are derived from the payloads), stage only the records and the payload words, and give the
 * seal of r0hip_prove_segment_trace_backs. Their records are checked in r0hip_worker_submit, as
 * r0hip_rv32im_inject_backs checks them; the r0hip_backs struct stays valid like the arrays.
 * Jobs of kind R0HIP_JOB_RECURSION_PROGRAM are recursion jobs from a resident program
 * (r0hip_recursion_program_create). Such a job is an r0hip_worker_program_job, the job struct
 * followed by the handle; r0hip_worker_submit takes the address of its `job` member (the
 * struct's own address) and r0hip_worker_wait hands that address back. r0hip_worker_job itself
 * keeps its size and every offset, so callers built against it are untouched. They use recursion.h_wom, h_cycles, h_iops and
 * the allow-list, ignore recursion.h_ctrl, stage no control group (the set's control buffer is
 * not grown for them) and give the seal of r0hip_prove_recursion_program with the worker's key
 * and stream_id = the ticket, which is also the kind-1 seal of the same input and ticket.
 * r0hip_worker_submit refuses a NULL handle, a handle whose suite or po2 differs from the job's
 * and n_cycles != the handle's code_rows; an accepted job holds a use count on the handle until
 * r0hip_worker_wait can hand it back (r0hip_recursion_program_destroy is refused meanwhile).
 * With verify, every seal goes through r0hip_verify_seal (recursion: against the
 * job's h_code_roots allow-list; a kind-3 job with n_code_roots = 0: against the handle's own
 * control id); a failed check sets "receipt verification failed: ..." on
 * that job alone.
 * r0hip_worker_wait returns the next finished job in completion order, each job exactly once.
 * *done = NULL with no error: the timeout passed (timeout_ms = 0 polls, < 0 waits without
 * limit) or nothing is outstanding; it never blocks when nothing is outstanding.
 * r0hip_worker_destroy runs everything submitted to completion (jobs not yet waited for keep
 * their results in their structs), joins the threads and returns the device memory: after
 * r0hip_trim, r0hip_mem_stats' live bytes are what they were before r0hip_worker_create.
 * submit and wait may be called from different threads; destroy must be the last call. */
typedef struct r0hip_worker r0hip_worker;
#define R0HIP_JOB_RV32IM_TRACE 0
#define R0HIP_JOB_RECURSION 1
#define R0HIP_JOB_RV32IM_BACKS 2
#define R0HIP_JOB_RECURSION_PROGRAM 3
typedef struct r0hip_recursion_input {
  const uint32_t* h_ctrl;        /* control group, 23 columns x 2^po2, host */
  const uint32_t* h_wom;         /* as r0hip_recursion_witgen takes them */
  size_t n_wom;
  const uint32_t* h_cycles;
  size_t n_cycles;
  const uint32_t* h_iops;
  size_t n_iops;
  const uint32_t* h_code_roots;  /* allow-list for the receipt check, 8 words each */
  size_t n_code_roots;           /* 0 = none */
} r0hip_recursion_input;
typedef struct r0hip_worker_job {
  uint32_t kind;                      /* R0HIP_JOB_* */
  int suite;
  uint32_t po2;
  r0hip_trace_input trace;            /* kind 0; kind 2: mode, h_global and preflight */
  const r0hip_bigint_back* h_bigint;  /* kind 0: the trace's BigInt backs (NULL, 0 if none) */
  size_t n_bigint;
  r0hip_recursion_input recursion;    /* kind 1; kind 3: all but h_ctrl */
  void* user;                         /* untouched */
  uint32_t* h_seal;                   /* out: the seal (seal_cap words), its length in seal_len */
  size_t seal_cap;
  size_t seal_len;
  uint32_t* h_mix_out;                /* out (optional): the mix words (36 rv32im, 20 recursion) */
  const char* error;                  /* out: NULL or a malloc'd message (free() it) */
  int verified;                       /* out: 1 when the seal passed r0hip_verify_seal */
  double verify_ms;                   /* out: host milliseconds of that check */
  double prove_ms;                    /* out: host milliseconds from a prover taking the job to its
                                         seal in host memory (the wait for its upload included) */
  uint64_t ticket;                    /* out: submission number, from 0 */
  const r0hip_backs* backs;           /* kind 2: the Back records (read for no other kind) */
} r0hip_worker_job;
/* a job of kind R0HIP_JOB_RECURSION_PROGRAM: r0hip_worker_job with the handle appended. Submit
 * &pj.job; a job of that kind is always read as this struct, a job of any other kind never is. */
typedef struct r0hip_worker_program_job {
  r0hip_worker_job job;                   /* kind 3; recursion: all but h_ctrl */
  const r0hip_recursion_program* program; /* the resident program */
} r0hip_worker_program_job;
/* a job of kind R0HIP_JOB_RECURSION_INPUT: a recursion job from a resident program and the
 * reference's `input` (r0hip_prove_recursion_program_input with the worker's key and stream_id =
 * the ticket, so its seal equals the kind-3 seal of the same input's preflight and ticket).
 * Submitted and handed back by the address of its `job` member, as kind 3 is; of job.recursion
 * only the allow-list is read. Submit refuses a NULL handle, a suite or po2 that is not the
 * handle's, po2 above max_po2, and takes a use count that lasts until the job can be handed back.
 * The preflight runs on the uploader thread while the provers work, into page-locked buffers of
 * the job's set (or on a pool thread, r0hip_worker_set_preflight_threads below); its failure lands
 * in this job's error alone. With verify and no allow-list the
 * seal is checked against the handle's control id. */
#define R0HIP_JOB_RECURSION_INPUT 4
typedef struct r0hip_worker_input_job {
  r0hip_worker_job job;                   /* kind 4 */
  const r0hip_recursion_program* program; /* the resident program */
  const uint32_t* h_input;                /* the input words, valid until the job is handed back */
  size_t n_input;
  uint32_t* h_output;                     /* out (optional): Preflight.output, output_cap words */
  size_t output_cap;
  size_t n_output;                        /* out: the output's length */
} r0hip_worker_input_job;
/* [drains] */
const char* r0hip_worker_create(r0hip_worker** out, uint32_t max_po2, uint32_t in_flight, int verify,
                                const uint32_t* h_noise_key);
/* [host-only] */
const char* r0hip_worker_submit(r0hip_worker* w, r0hip_worker_job* job);
/* [host-only] */
const char* r0hip_worker_wait(r0hip_worker* w, r0hip_worker_job** done, int64_t timeout_ms);
/* [drains] */
const char* r0hip_worker_destroy(r0hip_worker* w);
/* r0hip_set_witness_check for the worker's jobs: the switch applies to the jobs submitted after
 * the call and is recorded at r0hip_worker_submit (the job structs keep their layout); the prover
 * thread that takes a job sets its own mode to the job's. A job whose witness violates a
 * constraint gets "constraint check failed: ..." in its own error, verified = 0 and no seal; the
 * other jobs are untouched, and a passing job's seal is that of the switch off. */
/* [host-only] */
const char* r0hip_worker_set_witness_check(r0hip_worker* w, int on);
/* Kind-4 preflights on a pool of host threads. n = 0 (the default): the uploader thread runs each
 * kind-4 job's preflight itself, one at a time, and stages nothing else meanwhile. n = 1..8: n
 * pool threads run the preflights of queued kind-4 jobs ahead of the uploader, in ticket order,
 * each into one of n + in_flight + 1 slots of page-locked buffers (the look-ahead is bounded by
 * the slots); r0hip_worker_submit hands such a job to the pool as well as to the FIFO and still
 * touches no device; the uploader, on reaching the job, only waits for its preflight and points
 * the job's set at the slot, and the set's prover returns the slot once its stream has drained.
 * A pool thread never uses the device: no stream, no kernel, no copy, only the page-locked
 * allocation and free of its slot. A job whose handle has no plan yet when a pool thread takes it
 * is left to the uploader, which makes the plan and runs the preflight as with n = 0; call
 * r0hip_recursion_program_prepare_input first to have every job on the pool. Seals, mixes,
 * outputs, error messages and the order in which jobs start are those of n = 0. Refused, changing
 * nothing: w == NULL, n > 8, and a call while a job is outstanding (submitted and not yet handed
 * back by r0hip_worker_wait). *was (optional) receives the previous n. r0hip_worker_destroy joins
 * the pool threads and frees the slots. */
/* [host-only] */
const char* r0hip_worker_set_preflight_threads(r0hip_worker* w, uint32_t n, uint32_t* was);
/* Which way the worker's kind-4 preflights went, since r0hip_worker_create (peak_slots_in_use:
 * since the last change of n). Any thread, at any time before destroy. out_size must be
 * sizeof(r0hip_worker_stats). */
typedef struct r0hip_worker_stats {
  uint32_t preflight_threads, preflight_slots, peak_slots_in_use, reserved;
  uint64_t pool_jobs;      /* kind-4 preflights run by the pool */
  uint64_t inline_jobs;    /* kind-4 preflights run by the uploader */
  uint64_t slot_bytes;     /* page-locked bytes the slots hold now */
  double pool_busy_ms;               /* summed over pool threads, inside preflights */
  double uploader_preflight_ms;      /* uploader time inside inline preflights */
  double uploader_wait_preflight_ms; /* uploader time waiting for the pool */
} r0hip_worker_stats;
/* [host-only] */
const char* r0hip_worker_get_stats(r0hip_worker* w, r0hip_worker_stats* out, size_t out_size);

/* ---- seal verification (risc0/zkp/src/verify/mod.rs:500-560 `verify`, with merkle.rs:79-186,
 * fri.rs:36-155, read_iop.rs:20-84; rv32im seals lead with the version word 2,
 * circuit/rv32im/src/lib.rs:78-92) ----
 * Replays the transcript and checks the constraint validity equation poly_ext(z) ==
 * check(z) * ((3z)^N - 1) (mod.rs:340-394), every Merkle opening, every FRI fold, the final
 * FRI polynomial, that every field word read is canonical (read_field_elem_slice,
 * read_iop.rs:45-48) and the seal length. check_code (mod.rs:531): the code/control root is
 * written to h_code_root_out (8 words, if non-NULL), and when n_code_roots > 0 it must equal
 * one of the n_code_roots digests at h_code_roots (8 words each) — the recursion circuit's
 * control-id allow-list (zkvm/src/receipt/succinct.rs:143-157). Host-only: needs no GPU and
 * no r0hip_init. Returns NULL when the seal verifies (po2 of the segment in *po2_out, if
 * non-NULL), else the failed check. */
/* [host-only] */
const char* r0hip_verify_seal(const char* circuit, int suite, const uint32_t* seal, size_t seal_len,
                              const uint32_t* h_code_roots, size_t n_code_roots, uint32_t* h_code_root_out,
                              uint32_t* po2_out);
/* TESTING ONLY — never use it to accept a receipt. r0hip_verify_seal without the validity
 * equation and without a code-root check, for seals of synthetic witnesses (which do not
 * satisfy the constraints) in the parity tests. */
/* [host-only] */
const char* r0hip_testing_verify_seal_structure(const char* circuit, int suite, const uint32_t* seal,
                                                size_t seal_len, uint32_t* po2_out);
/* ---- the same check with the Merkle openings hashed on the device (opt-in) ----
 * where = R0HIP_VERIFY_HOST is r0hip_verify_seal itself: host-only, no GPU, no r0hip_init.
 * where = R0HIP_VERIFY_DEVICE keeps the transcript, the trees' top layers, the validity equation
 * and the FRI arithmetic on the host and hashes the seal's deferred openings (each row hash and
 * its path, 200-350 per seal) in one kernel on the calling thread's stream: the seal goes up once
 * through the thread's page-locked staging arena, the opening table and the results come from the
 * thread's pool, and the host compares each result with the tree's top layer, so the device
 * never decides a verdict. Verdicts, messages (the first failure in opening order), *po2_out and
 * the code root are those of the host check. Poseidon2 and SHA-256 run on the device;
 * Poseidon254 (suite 2) is accepted and runs the host openings, unless
 * r0hip_set_verify_device_poseidon254(1) was called (below): then its openings run on the device
 * too, one per lane. The device call always drains (also in deferred mode) and
 * the thread keeps no device memory afterwards. Any other `where` is an error. */
#define R0HIP_VERIFY_HOST 0
#define R0HIP_VERIFY_DEVICE 1
/* [drains] */
const char* r0hip_verify_seal_on(int where, const char* circuit, int suite, const uint32_t* seal, size_t seal_len,
                                 const uint32_t* h_code_roots, size_t n_code_roots, uint32_t* h_code_root_out,
                                 uint32_t* po2_out);
/* Poseidon254 openings on the device, behind a switch: process-wide, 0 by default, read at the
 * time of each check by r0hip_verify_seal_on and r0hip_testing_verify_seal_structure_on with
 * where = R0HIP_VERIFY_DEVICE, by r0hip_merkle_open_digests, and by verify = 2 in
 * r0hip_prove_segments, r0hip_prove_trace_segments and the worker's verifier thread. With 1 a
 * suite-2 seal's openings are hashed by one kernel (merkle_open_poseidon254, one opening per lane
 * on the library's own BN254 code); verdicts, messages, *po2_out and the code root do not
 * change. Each check reads the switch once, so a change made while a check runs takes effect
 * with the next check. Measured: a modest gain for one receipt
 * checked alone, none in a worker, where the switch trades receipt latency for host cores. With
 * 0 every call behaves as if the switch did not exist. Any value but 0 or 1 is an error naming
 * `on`. Needs no GPU and no r0hip_init. */
/* [host-only] */
const char* r0hip_set_verify_device_poseidon254(int on);
/* TESTING ONLY, as r0hip_testing_verify_seal_structure is, with the openings host or device. */
/* [drains] */
const char* r0hip_testing_verify_seal_structure_on(int where, const char* circuit, int suite, const uint32_t* seal,
                                                   size_t seal_len, uint32_t* po2_out);
/* The device step by itself: for each of n_open openings over the word buffer h_words (n_words
 * words), cur = hash_elems(suite, h_words + row_off, cols), then `levels` times cur =
 * hash_pair(other, cur) or hash_pair(cur, other) with `other` the next 8 words from h_words +
 * path_off: `other` goes left when the running index (index, then index >> 1, ...) is odd. index
 * is the leaf's heap index (row + rows of the tree). h_digests gets cur (8 words per opening),
 * h_status one word per opening: 0 computed; 2 (Poseidon2 only) a path digest word is >= p, the
 * case the verifier rejects as "non-canonical Poseidon2 digest word in seal" (the digest is then
 * written as zeros; the other openings are unaffected). The digests are byte for byte the host
 * verifier's (Poseidon2: sponge of rate 16, unpadded; SHA-256: the unpadded row hash over
 * little-endian words). suite 0 or 1; suite 2 is an error here unless
 * r0hip_set_verify_device_poseidon254(1) was called: then it is Poseidon254's unpadded_hash and
 * hash_pair, path digests are any 256-bit words (reduced mod r as the host's hash_pair reduces
 * them) and the status is always 0. Refused on the host before any device call, naming the
 * argument: a NULL array with a nonzero count, cols outside [1, 256], levels above 40, a row or
 * path range outside n_words, and (Poseidon2, Poseidon254) a row word >= p. Ranges may overlap
 * and openings may share rows. */
typedef struct r0hip_opening {
  uint64_t row_off;  /* first word of the row in h_words */
  uint64_t path_off; /* first word of the path: 8 words per level */
  uint64_t index;    /* heap index of the leaf */
  uint32_t cols;     /* row length in words, 1..256 */
  uint32_t levels;   /* path length in digests, 0..40 */
} r0hip_opening;
/* [drains] */
const char* r0hip_merkle_open_digests(int suite, const uint32_t* h_words, size_t n_words, const r0hip_opening* h_open,
                                      size_t n_open, uint32_t* h_digests, uint32_t* h_status);

/* PolyExt::poly_ext of the circuit (its generated poly_ext.rs, called at mod.rs:356-386): the
 * constraint polynomial at the out-of-domain point. h_mix (mix_size) and h_global
 * (output_size) are Montgomery words, h_eval_u one FpExt (4 words) per tap in tap order,
 * h_poly_mix one FpExt; the result FpExt goes to h_out. Host-only. */
/* [host-only] */
const char* r0hip_poly_ext(const char* circuit, const uint32_t* h_mix, const uint32_t* h_global,
                           const uint32_t* h_eval_u, const uint32_t* h_poly_mix, uint32_t* h_out);

/* ---- constraint check on the trace rows (a diagnostic, opt-in) ----
 * The circuit's constraint polynomial vanishes on every row of a valid trace, the ZK rows
 * included. r0hip_constraint_rows evaluates it (poly_fp of the reference, with poly_mix given) on
 * the 2^po2 rows of the witness groups as they are: d_code, d_data and d_accum are the device
 * matrices r0hip_prove_segment takes (column-major, 2^po2 rows; the groups in their final form,
 * zeroized and accumulated), d_mix and d_global the device arrays r0hip_eval_check takes. A tap is
 * read at (row - back) mod 2^po2, so a `back` at or above 2^po2 wraps. h_poly_mix: four Montgomery
 * words (one FpExt); NULL draws them with getrandom(2). d_out (may be NULL): the value of every
 * row, one FpExt (4 words, AoS) per row, 2^po2 * 4 words, bit for bit the reference's poly_fp on
 * that row's taps. The report: bad_rows = how many rows are nonzero, first_row the smallest of
 * them, rows[0 .. n_rows) the first n_rows = min(bad_rows, 16) in ascending order (0xFFFFFFFF
 * beyond, and first_row = 0xFFFFFFFF when there is none), first_term = r0hip_constraint_term on
 * first_row, whose taps the call gathers to the host (-1 when no row is bad). A violated witness
 * is a successful call with bad_rows > 0, not an error. po2 is 2..24. Refused on the host, naming
 * the argument, before any device call: a NULL pointer (all but h_poly_mix and d_out), an unknown
 * circuit, po2 out of range.
 * Not part of soundness: a violated row gives zero for a random poly_mix with probability at most
 * (number of terms) / p^4, and the check says nothing about a prover that goes on to commit
 * other values. It answers "is the witness wrong, or the polynomial side?" in a quarter of
 * eval_check's points, before the proof is paid for.
 * r0hip_constraint_term: the host half alone; needs no GPU and no r0hip_init. h_taps: one row's
 * tap values, one Montgomery word per tap in tap order (the order of r0hip_poly_ext's h_eval_u);
 * h_mix, h_global, h_poly_mix as r0hip_poly_ext takes them. *term = the value id, in the
 * committed risc0_amd/circuits/<circuit>.poly.ir, of the first violated term: the accumulate
 * chain that ends at the `r` record is walked in chain order for the first `a`/`b` record whose
 * added amount is nonzero; for a `b` (a guarded block) the walk repeats inside its inner chain
 * and the innermost id is returned. -1 when the row satisfies every constraint. */
typedef struct r0hip_constraint_report {
  uint64_t bad_rows;   /* rows whose constraint value is nonzero */
  uint32_t first_row;  /* the smallest of them, 0xFFFFFFFF if none */
  int32_t first_term;  /* r0hip_constraint_term on first_row, -1 if none */
  uint32_t n_rows;     /* entries of rows[] in use: min(bad_rows, 16) */
  uint32_t rows[16];   /* the first bad rows, ascending */
} r0hip_constraint_report;
/* [drains] */
const char* r0hip_constraint_rows(const char* circuit, uint32_t po2, const uint32_t* d_code, const uint32_t* d_data,
                                  const uint32_t* d_accum, const uint32_t* d_mix, const uint32_t* d_global,
                                  const uint32_t* h_poly_mix, uint32_t* d_out, r0hip_constraint_report* report);
/* [host-only] */
const char* r0hip_constraint_term(const char* circuit, const uint32_t* h_taps, const uint32_t* h_mix,
                                  const uint32_t* h_global, const uint32_t* h_poly_mix, int32_t* term);

/* ---- circuits compiled in: the shipped ones, the demo circuit, build-time plug-ins ----
 * The circuit-generic entry points (r0hip_eval_check, r0hip_poly_ext, r0hip_constraint_rows,
 * r0hip_constraint_term, r0hip_prove_segment, r0hip_prove_segment_cb, r0hip_prove_segments,
 * r0hip_verify_seal*, the testing variants) take any name the library was built with: "rv32im",
 * "recursion", "demo", and every circuit of the directories given to the build as
 * EXTRA_CIRCUIT_DIRS ("Adding a circuit / checking a card"), and every circuit
 * registered at run time (r0hip_circuit_register, below). An unknown name's error lists the names
 * compiled in and, once there are any, the registered ones after them
 * ("(compiled in: rv32im, recursion, demo; registered: x)"); r0hip_circuit_info with a NULL circuit
 * lists both sets, compiled in first. The rv32im version word and the two device accumulations
 * (r0hip_prove_segment_accum) stay tied to their circuits' names.
 * r0hip_circuit_info: what a caller needs to size a circuit's buffers. circuit = NULL: the names,
 * space-separated in build order, into names (names_cap bytes, NUL-terminated; too small is an
 * error); out is not written. Otherwise *out (out_size = sizeof(r0hip_circuit_desc)) describes the
 * named circuit and names, if given, receives its name. Host-only. */
typedef struct r0hip_circuit_desc {
  uint32_t group_sizes[3]; /* columns of accum, code, data */
  uint32_t mix_size;       /* words drawn after the data commit */
  uint32_t output_size;    /* words of the global (output) buffer */
  uint32_t n_taps;         /* taps, the length of r0hip_poly_ext's h_eval_u in FpExt */
  uint8_t info[16];        /* the circuit's CircuitInfo bytes */
} r0hip_circuit_desc;
/* [host-only] */
const char* r0hip_circuit_info(const char* circuit, r0hip_circuit_desc* out, size_t out_size, char* names,
                               size_t names_cap);

/* ---- circuits registered at run time ----
 * r0hip_circuit_register: a circuit's tables handed over while the process runs, for a circuit
 * the library was not built with ("A circuit at run time"). From then on every
 * circuit-generic entry point above takes the name, as it takes a compiled-in one; eval_check and
 * the constraint-rows check run an interpreter of the constraint program on the device, which is
 * several times slower than the kernels a build generates. The fields mirror the tables of a
 * compiled-in circuit (tools/gen_circuits_inc.py writes the same arrays from <name>.taps.json and
 * <name>.poly.ir):
 *   taps        n_taps x {offset, back, group, combo, skip}, sorted by group, offset, back
 *   eval_args   per eval_check argument: 0 accum, 1 code, 2 data, -1 mix, -2 global
 *   ir          n_ir records {op, dst, a, b, c, d}, op the index into "celg+-*abr", dst dense
 *               from 0 (the `r` record, last, names the result in dst): c {word}, e {4 words}
 *               (Montgomery, below p), l {tap index}, g {0 mix | 1 global, word index},
 *               + - * {id, id}, a {acc, x, power}, b {acc, x, y, power}
 * t_size = sizeof(r0hip_circuit_tables). Everything is copied; the copy lives until the process
 * ends and there is no way to take a circuit out (proofs in flight hold it). Safe from several
 * threads; needs no GPU and no r0hip_init. Refused, with the field named and the registry
 * unchanged: a name that is not a C identifier of at most 31 characters or is taken; more than 64
 * registrations; taps out of order or whose skips do not tile the registers; combo_begin,
 * group_begin (n_groups = 3) or group_sizes that disagree with the taps; eval_args outside the
 * five values or more than 16 of them; mix_size or output_size of 2^24 or more; n_ir = 0 or above
 * 2^20; and in ir: an op outside the ten, a dst that is not dense, an operand id that is not below
 * its record's dst, no `r` record or one that is not last, an l whose tap index is not below
 * n_taps or whose group eval_args lacks, a g whose word index is not below mix_size or
 * output_size, an a or b whose power is not below n_poly_mix or whose acc is not an FpExt value
 * (c, l, g are Fp; e, a, b FpExt; + - * the wider operand's), a constant word of p or more.
 * The rv32im version word, the two device accumulations (r0hip_prove_segment_accum refuses a
 * registered circuit) and the witness generators stay tied to the compiled-in names. */
typedef struct r0hip_circuit_tables {
  const char* name;
  const uint32_t* taps;
  size_t n_taps;
  const uint32_t* combo_taps;
  size_t n_combo_taps;
  const uint32_t* combo_begin; /* combos_count + 1 */
  size_t combos_count;
  const uint32_t* group_begin; /* n_groups + 1 */
  size_t n_groups;
  const uint32_t* group_sizes; /* n_groups */
  const uint32_t* poly_mix_powers;
  size_t n_poly_mix;
  uint8_t info[16]; /* the circuit's CircuitInfo bytes */
  size_t mix_size;
  size_t output_size;
  const int32_t* eval_args;
  size_t n_eval_args;
  const uint32_t* ir; /* 6 * n_ir words */
  size_t n_ir;
} r0hip_circuit_tables;
/* [host-only] */
const char* r0hip_circuit_register(const r0hip_circuit_tables* t, size_t t_size);

/* ---- circuit modules: a circuit's generated kernels loaded at run time ----
 * There are three ways to bring a circuit in, and r0hip_circuit_backend tells them apart:
 *   0  compiled in (the shipped circuits, the demo, EXTRA_CIRCUIT_DIRS): the generated kernels,
 *      in a library built for them; for a deployment that builds its own libr0hip.so;
 *   1  registered (r0hip_circuit_register): no build at all, the device interprets the program,
 *      several times slower; for developing a circuit;
 *   2  a module (r0hip_circuit_load): the same generated kernels as 0, compiled once into a
 *      shared object of their own (`make -C risc0_amd/csrc module NAME=x DIR=dir
 *      OUT=path/x.r0mod.so`, r0hip_module.h) and handed to a stock library while it runs; for
 *      proving a circuit of one's own at production speed.
 * r0hip_circuit_load opens path with dlopen(RTLD_NOW | RTLD_LOCAL), reads the descriptor its one
 * exported function returns, and checks, in this order: the ABI number and the three struct
 * sizes the module was compiled with (both values are printed), its architecture against the
 * library's, its tables exactly as r0hip_circuit_register checks them (the same words, the field
 * named), and what its kernels say of themselves (info() and rows_info(): nargs against
 * eval_args, every column inside the witness group it names, every folded product's power index
 * below npm, npm within poly_mix_powers, mat_fp, mat_ext and kernels within the driver's
 * limits). Only then is the circuit appended to the registry, under the name in its tables,
 * which name_out (may be NULL; name_cap >= 32 otherwise) receives. From then on every
 * circuit-generic entry point takes the name and runs the module's kernels, word for word as a
 * compiled-in circuit's; the interpreter plays no part. A refusal names the path and the reason
 * ("r0hip_circuit_load: <path>: <reason>"), closes the file again and leaves the registry
 * unchanged: a file that is missing or no shared object (the loader's message is quoted), no
 * entry symbol, a name that is taken (a second load of the same file falls here), the 64-entry
 * limit it shares with r0hip_circuit_register, and the checks above. A loaded module is never
 * closed. Loading runs the module's code, exactly as linking it would. Safe from several
 * threads; needs no GPU and no r0hip_init. What refuses a registered circuit refuses a loaded
 * one with the same words (r0hip_prove_segment_accum, the witness generators, the rv32im version
 * word stay tied to the compiled-in names).
 * In the unknown-circuit message and in r0hip_circuit_info's list, loaded names stand among the
 * registered ones in the order they arrived, and the message's word for both is "registered"
 * ("(compiled in: rv32im, recursion, demo; registered: x, y)"). */
/* [host-only] */
const char* r0hip_circuit_load(const char* path, char* name_out, size_t name_cap);
/* *kind = 0 compiled in, 1 registered (interpreted), 2 a module; an unknown name is an error. */
/* [host-only] */
const char* r0hip_circuit_backend(const char* circuit, int* kind);

/* TESTING ONLY: the points one launch of the interpreter takes on the calling thread, in place of
 * the chunk its slot-file budget gives; 0 = the budget's own choice, which
 * every new thread starts with. *was (may be NULL) = the previous value. */
/* [host-only] */
const char* r0hip_testing_set_interp_chunk(uint32_t points, uint32_t* was);

/* r0hip_prove_segment with the accum group made after the mix is drawn, for a circuit whose
 * accumulation the library does not have. The library commits code and data, draws the
 * circuit's mix_size words, allocates d_accum (2^po2 x group_sizes[0] words, filled with
 * 0xFFFFFFFF), drains its stream and calls accum(user, h_mix, d_accum, stream) on the calling
 * thread; then it zeroizes the group, runs the witness check if that mode is on, commits the
 * group and finishes the proof. The function may queue work on stream (a hipStream_t, the
 * calling thread's) or write d_accum through synchronous copies of its own, the r0hip_memcpy_*
 * and per-op entry points included; it must not prove or verify on this thread. It returns NULL,
 * or a message: the call then fails with "accum callback: <message>" (the string stays the
 * callback's; the library copies it). d_accum is the library's and is gone after the call. For
 * rv32im and recursion a callback that copies in the group r0hip_prove_segment was given yields
 * that call's seal, word for word. Proof streams, deferred mode and the memory hand-back are
 * r0hip_prove_segment's. h_mix_out (may be NULL): the mix words. */
typedef const char* (*r0hip_accum_fn)(void* user, const uint32_t* h_mix, uint32_t* d_accum, void* stream);
/* [drains] */
const char* r0hip_prove_segment_cb(const char* circuit, int suite, uint32_t po2, const uint32_t* d_code,
                                   const uint32_t* d_data, r0hip_accum_fn accum, void* user, uint32_t* d_global,
                                   int write_version, uint32_t version, uint32_t* h_seal, size_t seal_cap,
                                   size_t* seal_len, uint32_t* h_mix_out);

/* ---- the demo circuit and the card self-test ----
 * "demo" (risc0_amd/circuits/demo.*, written by tools/gen_demo_circuit.py) is a small circuit of
 * this library's own whose valid witness the library can make: code = the selectors first, on,
 * last; data = a, b, s with (a, b)[i] = (b, a + b)[i - 1] and s = a * b on the n_active rows;
 * accum = one FpExt, the running sum of m * a with m the four mix words; global = a[0], b[0],
 * b[n_active - 1]. Every constraint carries a selector that is 0 above n_active, so those rows
 * of data and accum may hold anything (ZK noise).
 * r0hip_demo_witness: d_code (3 columns x 2^po2 rows, every row) and d_global (3 words) are
 * written; of d_data (3 columns) only the rows below n_active: fill the group with noise first
 * (r0hip_fill_chacha20). a0, b0: Montgomery words below p. 1 <= n_active <= 2^po2, po2 2..24.
 * r0hip_demo_accum: the rows below n_active of d_accum (4 columns) from d_data's column a and
 * h_mix (4 Montgomery words); what an r0hip_prove_segment_cb callback for "demo" queues. */
/* [queues] */
const char* r0hip_demo_witness(uint32_t po2, size_t n_active, uint32_t a0, uint32_t b0, uint32_t* d_code,
                               uint32_t* d_data, uint32_t* d_global);
/* [queues] */
const char* r0hip_demo_accum(uint32_t po2, size_t n_active, const uint32_t* d_data, const uint32_t* h_mix,
                             uint32_t* d_accum);

/* r0hip_selftest: a health check of the card this thread is on, before it takes jobs. For every
 * hash suite in suites_mask (bit R0HIP_POSEIDON2, R0HIP_SHA256, R0HIP_POSEIDON254), at 2^po2 rows:
 *   a  the demo witness is made on the device, proved through r0hip_prove_segment_cb and the seal
 *      checked by r0hip_verify_seal (validity equation included) and again with the openings on
 *      the device (R0HIP_VERIFY_DEVICE);
 *   b  r0hip_constraint_rows finds no bad row in that witness, and exactly the two rows that tap
 *      it after one word of column a is changed in a copy;
 *   c  the seal with one word changed is rejected by the verifier.
 * Every negative case is a verdict of a check, never a device fault. The report (out_size =
 * sizeof(r0hip_selftest_report)) has, per suite, the checks that passed (bit 0 a, 1 b, 2 c), the
 * milliseconds of each and the seal's length in words; suites not asked for are zero. Returns
 * NULL only when every check of every suite asked for passed, else a message naming the first
 * that did not. Refused on the host: a mask of 0 or above 7, po2 outside 8..24, a NULL report,
 * an out_size that is not the struct's. The thread keeps no device memory afterwards. */
typedef struct r0hip_selftest_suite {
  uint32_t passed;   /* bit 0: a, bit 1: b, bit 2: c */
  uint32_t seal_len; /* words of the seal of check a */
  double ms[3];      /* wall time of a, b, c */
} r0hip_selftest_suite;
typedef struct r0hip_selftest_report {
  r0hip_selftest_suite suite[3]; /* by suite id */
} r0hip_selftest_report;
/* [drains] */
const char* r0hip_selftest(uint32_t suites_mask, uint32_t po2, r0hip_selftest_report* out, size_t out_size);

/* kernel-level timing with HIP events on the library stream: enable, run, then read
 * "name=total_ms:calls:alg_bytes;..." (alg_bytes = algorithmic HBM bytes) */
/* [drains] */
const char* r0hip_set_kernel_timing(int on);
/* [drains] */
const char* r0hip_kernel_times(char* buf, size_t cap);
/* per-phase device timings (ms) of the last r0hip_prove_segment, as "name=ms;..." */
/* [drains] */
const char* r0hip_last_profile(char* buf, size_t cap);

/* Device-memory accounting, replacing the reference HAL's MemoryTracker
 * (risc0/zkp/src/hal/mod.rs:292-317, reported as the datasheet's `ram`,
 * risc0/zkvm/examples/datasheet.rs:251). out[5] = {live bytes (buffers handed out),
 * peak live bytes, reserved bytes (held from hipMalloc incl. the free pool), peak
 * reserved bytes, number of hipMalloc calls}. Peaks are since the last reset. Host-only. */
/* [host-only] */
const char* r0hip_mem_stats(uint64_t* out);
/* [host-only] */
const char* r0hip_mem_reset_peak(void);
/* Release the idle device memory the library holds: the calling thread's free pool and
 * the blocks exited threads left (pool and scratch). Blocks in use are untouched. For a
 * caller switching segment sizes, and for tests that need a clean pool. */
/* [drains] */
const char* r0hip_trim(void);

#ifdef __cplusplus
}
#endif
#endif /* R0HIP_H */
