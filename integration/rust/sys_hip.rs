// risc0/sys/src/hip.rs — raw bindings of libr0hip (include/r0hip.h), behind `feature = "hip"`.
//
// Replaces for the HIP backend what risc0/sys/src/cuda.rs:19-80 (sppark_* and
// supra_poly_divide) and the risc0_zkp_cuda_* block bound by risc0/zkp/src/hal/cuda.rs
// provide for CUDA, plus the device/memory calls the `cust` crate makes there (cust does
// not run on ROCm). Every function returns NULL on success or a malloc'd message; wrap the
// call in `risc0_sys::ffi_wrap` (risc0/sys/src/lib.rs:53-75), which frees it.
//
// NOT COMPILED IN THIS REPOSITORY: the image has no Rust toolchain. The declarations are
// checked against include/r0hip.h by tests/test_integration_sources.py (every r0hip_* symbol
// the header declares is bound here with the same arity).
//
// build.rs of risc0-sys, `hip` feature (the kernels are prebuilt for gfx950 by
// `python -c "import __graft_entry__ as g; g.build()"`):
//     if env::var("CARGO_FEATURE_HIP").is_ok() {
//         let dir = env::var("R0HIP_LIB_DIR").expect("R0HIP_LIB_DIR: directory of libr0hip.so");
//         println!("cargo:rustc-link-search=native={dir}");
//         println!("cargo:rustc-link-lib=dylib=r0hip");
//         println!("cargo:rerun-if-env-changed=R0HIP_LIB_DIR");
//     }

use std::os::raw::{c_char, c_int, c_void};

/// Hash suite selectors of r0hip_hash_rows / r0hip_hash_fold / r0hip_prove_segment.
pub const R0HIP_POSEIDON2: c_int = 0;
pub const R0HIP_SHA256: c_int = 1;
pub const R0HIP_POSEIDON254: c_int = 2;

/// One Back::BigInt record of the rv32im preflight trace (struct r0hip_bigint_back).
/// struct r0hip_constraint_report: what r0hip_constraint_rows found on the trace rows.
#[repr(C)]
pub struct R0HipConstraintReport {
    pub bad_rows: u64,
    pub first_row: u32,
    pub first_term: i32,
    pub n_rows: u32,
    pub rows: [u32; 16],
}

/// struct r0hip_circuit_desc: the sizes of a circuit compiled into the library.
#[repr(C)]
pub struct R0HipCircuitDesc {
    pub group_sizes: [u32; 3],
    pub mix_size: u32,
    pub output_size: u32,
    pub n_taps: u32,
    pub info: [u8; 16],
}

/// struct r0hip_circuit_tables: a circuit handed to r0hip_circuit_register at run time (the
/// library copies every array).
#[repr(C)]
pub struct R0HipCircuitTables {
    pub name: *const c_char,
    pub taps: *const u32,
    pub n_taps: usize,
    pub combo_taps: *const u32,
    pub n_combo_taps: usize,
    pub combo_begin: *const u32,
    pub combos_count: usize,
    pub group_begin: *const u32,
    pub n_groups: usize,
    pub group_sizes: *const u32,
    pub poly_mix_powers: *const u32,
    pub n_poly_mix: usize,
    pub info: [u8; 16],
    pub mix_size: usize,
    pub output_size: usize,
    pub eval_args: *const i32,
    pub n_eval_args: usize,
    pub ir: *const u32,
    pub n_ir: usize,
}

/// r0hip_accum_fn: fills the accum group once the mix is known; NULL, or a message that fails the proof.
pub type R0HipAccumFn = Option<
    unsafe extern "C" fn(user: *mut c_void, h_mix: *const u32, d_accum: *mut u32, stream: *mut c_void) -> *const c_char,
>;

/// struct r0hip_selftest_suite / r0hip_selftest_report: what r0hip_selftest found, per hash suite.
#[repr(C)]
pub struct R0HipSelftestSuite {
    pub passed: u32,
    pub seal_len: u32,
    pub ms: [f64; 3],
}
#[repr(C)]
pub struct R0HipSelftestReport {
    pub suite: [R0HipSelftestSuite; 3],
}

#[repr(C)]
pub struct R0HipBigIntBack {
    pub row: u32,
    pub poly_op: u32,
    pub coeff: u32,
    pub bytes: [u8; 16],
}

/// A preflight trace as a job of r0hip_prove_trace_segments takes it (struct r0hip_trace_input):
/// host pointers; `preflight` has the repr(C) layout of risc0_circuit_rv32im_sys::RawPreflightTrace.
#[repr(C)]
pub struct R0HipTraceInput {
    pub mode: u32,
    pub h_global: *const u32,
    pub h_inj_index: *const u32,
    pub inj_rows: usize,
    pub h_inj_offsets: *const u32,
    pub h_inj_values: *const u32,
    pub preflight: risc0_circuit_rv32im_sys::RawPreflightTrace,
}

/// One job of r0hip_prove_segments: host witness groups in, seal out (struct r0hip_segment_job).
#[repr(C)]
pub struct R0HipSegmentJob {
    pub h_code: *const u32,
    pub h_data: *const u32,
    pub h_accum: *const u32,
    pub h_global: *const u32,
    pub h_bigint: *const R0HipBigIntBack,
    pub n_bigint: usize,
    pub h_seal: *mut u32,
    pub seal_cap: usize,
    pub seal_len: usize,
    pub h_mix_out: *mut u32,
    pub error: *const c_char,
}

/// One job of r0hip_prove_trace_segments (struct r0hip_trace_job): the rv32im prove_core of one
/// preflight trace; seal out, and with `verify` the receipt check's outcome.
#[repr(C)]
pub struct R0HipTraceJob {
    pub trace: R0HipTraceInput,
    pub h_bigint: *const R0HipBigIntBack,
    pub n_bigint: usize,
    pub h_seal: *mut u32,
    pub seal_cap: usize,
    pub seal_len: usize,
    pub h_mix_out: *mut u32,
    pub error: *const c_char,
    pub verified: c_int,
    pub verify_ms: f64,
    pub prove_ms: f64,
}

/// The GPU worker's handle (struct r0hip_worker): opaque, made by r0hip_worker_create.
#[repr(C)]
pub struct R0HipWorker {
    _private: [u8; 0],
}

/// Job kinds of R0HipWorkerJob (R0HIP_JOB_*).
pub const R0HIP_JOB_RV32IM_TRACE: u32 = 0;
pub const R0HIP_JOB_RECURSION: u32 = 1;
pub const R0HIP_JOB_RV32IM_BACKS: u32 = 2;
pub const R0HIP_JOB_RECURSION_PROGRAM: u32 = 3;
pub const R0HIP_JOB_RECURSION_INPUT: u32 = 4;

/// Forms of the code words r0hip_recursion_program_create takes (R0HIP_CODE_*).
pub const R0HIP_CODE_ENCODED: c_int = 0; // plain u32 words of a .zkr (Elem::from per word)
pub const R0HIP_CODE_MONTGOMERY: c_int = 1; // Program.code: canonical Montgomery words

/// A recursion program resident on the device (struct r0hip_recursion_program, opaque).
#[repr(C)]
pub struct R0HipRecursionProgram {
    _private: [u8; 0],
}

/// Record kinds of R0HipBack (R0HIP_BACK_*) and their payload sizes in words.
pub const R0HIP_BACK_ECALL: u32 = 1; // 3: s0, s1, s2
pub const R0HIP_BACK_POSEIDON2: u32 = 2; // 39: Poseidon2State::as_array
pub const R0HIP_BACK_SHA2: u32 = 3; // 10: Sha2State::fp_array, then a, e, w
pub const R0HIP_BACK_BIGINT: u32 = 4; // 22: BigIntState::as_array

/// One row's Back record (struct r0hip_back): `word` is the index of its payload's first word.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct R0HipBack {
    pub row: u32,
    pub kind: u32,
    pub word: u32,
}

/// The injector as the preflight's Back records (struct r0hip_backs): what build_injector reads,
/// not what it writes. Payload words are plain u32, as the reference's arrays hold them.
#[repr(C)]
pub struct R0HipBacks {
    pub recs: *const R0HipBack,
    pub n: usize,
    pub words: *const u32,
    pub n_words: usize,
    pub inj_rows: usize,
}

/// One recursion job's host arrays (struct r0hip_recursion_input): the control group and the
/// preflight as r0hip_recursion_witgen takes them, and the allow-list of its receipt check.
#[repr(C)]
pub struct R0HipRecursionInput {
    pub h_ctrl: *const u32,
    pub h_wom: *const u32,
    pub n_wom: usize,
    pub h_cycles: *const u32,
    pub n_cycles: usize,
    pub h_iops: *const u32,
    pub n_iops: usize,
    pub h_code_roots: *const u32,
    pub n_code_roots: usize,
}

/// One job of the GPU worker (struct r0hip_worker_job): an rv32im prove_core from a preflight
/// trace (kind 0), the same from its Back records (kind 2, `backs`) or a recursion proof (kind
/// 1). It must not move, and its host arrays must
/// stay valid, from r0hip_worker_submit until r0hip_worker_wait hands it back.
#[repr(C)]
pub struct R0HipWorkerJob {
    pub kind: u32,
    pub suite: c_int,
    pub po2: u32,
    pub trace: R0HipTraceInput,
    pub h_bigint: *const R0HipBigIntBack,
    pub n_bigint: usize,
    pub recursion: R0HipRecursionInput,
    pub user: *mut c_void,
    pub h_seal: *mut u32,
    pub seal_cap: usize,
    pub seal_len: usize,
    pub h_mix_out: *mut u32,
    pub error: *const c_char,
    pub verified: c_int,
    pub verify_ms: f64,
    pub prove_ms: f64,
    pub ticket: u64,
    pub backs: *const R0HipBacks,
}

/// A job of kind R0HIP_JOB_RECURSION_PROGRAM (struct r0hip_worker_program_job): the job with the
/// handle appended. Submit `&mut pj.job`; r0hip_worker_wait hands that address back.
#[repr(C)]
pub struct R0HipWorkerProgramJob {
    pub job: R0HipWorkerJob,
    pub program: *const R0HipRecursionProgram,
}

/// A job of kind R0HIP_JOB_RECURSION_INPUT (struct r0hip_worker_input_job): the job, the handle
/// and the words RecursionProver::prove calls `input`. Submit `&mut ij.job`.
#[repr(C)]
pub struct R0HipWorkerInputJob {
    pub job: R0HipWorkerJob,
    pub program: *const R0HipRecursionProgram,
    pub h_input: *const u32,
    pub n_input: usize,
    pub h_output: *mut u32,
    pub output_cap: usize,
    pub n_output: usize,
}

/// Which way the worker's kind-4 preflights went (struct r0hip_worker_stats).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct R0HipWorkerStats {
    pub preflight_threads: u32,
    pub preflight_slots: u32,
    pub peak_slots_in_use: u32,
    pub reserved: u32,
    pub pool_jobs: u64,
    pub inline_jobs: u64,
    pub slot_bytes: u64,
    pub pool_busy_ms: f64,
    pub uploader_preflight_ms: f64,
    pub uploader_wait_preflight_ms: f64,
}

/// What r0hip_recursion_program_prepare_input made (struct r0hip_recursion_input_info).
#[repr(C)]
pub struct R0HipRecursionInputInfo {
    pub prepared: u32,
    pub n_runs: u32,
    pub bucket_runs: [u32; 9],
    pub n_wom: usize,
    pub n_iops: usize,
    pub n_output: usize,
    pub n_input: u64,
    pub plan_device_bytes: u64,
    pub plan_host_bytes: u64,
}

/// One Merkle opening over a word buffer (struct r0hip_opening): the row at `row_off`, `levels`
/// path digests at `path_off`, sides read from the leaf's heap index.
#[repr(C)]
pub struct R0HipOpening {
    pub row_off: u64,
    pub path_off: u64,
    pub index: u64,
    pub cols: u32,
    pub levels: u32,
}

/// `where` of r0hip_verify_seal_on: the openings on host threads, or hashed on the device.
pub const R0HIP_VERIFY_HOST: c_int = 0;
pub const R0HIP_VERIFY_DEVICE: c_int = 1;
/// `verify` of r0hip_prove_trace_segments and r0hip_worker_create: receipts checked with the
/// openings on the device (any other nonzero value: on the host).
pub const R0HIP_VERIFY_RECEIPTS_DEVICE: c_int = 2;

#[link(name = "r0hip")]
unsafe extern "C" {
    // ---- device and memory (cust's role in hal/cuda.rs:235-421) ----
    pub fn r0hip_init(device_ordinal: c_int) -> *const c_char;
    pub fn r0hip_device_info(name: *mut c_char, name_cap: usize, total_mem: *mut u64) -> *const c_char;
    pub fn r0hip_alloc(d_ptr: *mut *mut c_void, bytes: usize) -> *const c_char;
    pub fn r0hip_free(d_ptr: *mut c_void) -> *const c_char;
    pub fn r0hip_memset32(d_dst: *mut c_void, value: u32, count: usize) -> *const c_char;
    pub fn r0hip_memcpy_h2d(d_dst: *mut c_void, h_src: *const c_void, bytes: usize) -> *const c_char;
    pub fn r0hip_memcpy_d2h(h_dst: *mut c_void, d_src: *const c_void, bytes: usize) -> *const c_char;
    pub fn r0hip_memcpy_d2d(d_dst: *mut c_void, d_src: *const c_void, bytes: usize) -> *const c_char;
    pub fn r0hip_host_alloc(h_ptr: *mut *mut c_void, bytes: usize) -> *const c_char;
    pub fn r0hip_host_free(h_ptr: *mut c_void) -> *const c_char;
    pub fn r0hip_synchronize() -> *const c_char;
    // the calling thread's completion mode (device-only calls return with their work queued) and
    // its call counters {calls, drained, queued}
    pub fn r0hip_set_deferred(on: c_int, was: *mut c_int) -> *const c_char;
    pub fn r0hip_call_stats(out: *mut u64) -> *const c_char;
    // {launched, in the program}: the kernels of this thread's last eval_check after its zero scan
    pub fn r0hip_eval_check_launched(out: *mut c_int) -> *const c_char;
    // the zero scan on its own: bit c of *h_mask = column c of the column-major matrix is all zero
    pub fn r0hip_testing_zero_scan(d_matrix: *const u32, cols: usize, words: usize, h_mask: *mut u64) -> *const c_char;
    // streams one proof of the calling thread may use (1..3; for a worker proving one task at a time)
    pub fn r0hip_set_proof_streams(n: u32, was: *mut u32) -> *const c_char;
    // the calling thread's witness check: the provers evaluate the constraint polynomial on the
    // trace rows before the accum commit and fail with "constraint check failed: ..." (opt-in)
    pub fn r0hip_set_witness_check(on: c_int, was: *mut c_int) -> *const c_char;
    pub fn r0hip_free_error(err: *const c_char);
    // a device-to-host copy beside later calls (the HAL's node-heap mirrors, hal_hip.rs)
    pub fn r0hip_memcpy_d2h_start(h_dst: *mut c_void, d_src: *const c_void, bytes: usize,
                                  h_copy: *mut *mut c_void) -> *const c_char;
    pub fn r0hip_copy_finish(h_copy: *mut c_void, block: c_int, done: *mut c_int) -> *const c_char;

    // ---- NTT family (sppark_batch_expand/NTT/iNTT/zk_shift, cuda_batch_bit_reverse) ----
    pub fn r0hip_batch_expand_into_evaluate_ntt(
        d_out: *mut u32,
        d_in: *const u32,
        count: usize,
        lg_out: u32,
        expand_bits: u32,
    ) -> *const c_char;
    pub fn r0hip_batch_interpolate_ntt(d_io: *mut u32, count: usize, lg_size: u32) -> *const c_char;
    pub fn r0hip_zk_shift(d_io: *mut u32, count: usize, lg_size: u32) -> *const c_char;
    pub fn r0hip_batch_bit_reverse(d_io: *mut u32, count: usize, lg_size: u32) -> *const c_char;

    // ---- polynomial ops ----
    pub fn r0hip_batch_evaluate_any(
        d_out: *mut u32,
        d_coeffs: *const u32,
        poly_count: usize,
        lg_poly_size: u32,
        d_which: *const u32,
        d_xs: *const u32,
        eval_count: usize,
    ) -> *const c_char;
    pub fn r0hip_mix_poly_coeffs(
        d_out: *mut u32,
        d_in: *const u32,
        h_combos: *const u32,
        h_mix_start: *const u32,
        h_mix: *const u32,
        input_size: usize,
        count: usize,
    ) -> *const c_char;
    pub fn r0hip_fri_fold(d_out: *mut u32, d_in: *const u32, h_mix: *const u32, count: usize) -> *const c_char;
    pub fn r0hip_combos_prepare(
        d_combos: *mut u32,
        h_coeff_u: *const u32,
        combo_count: usize,
        cycles: usize,
        h_reg_sizes: *const u32,
        h_reg_combo_ids: *const u32,
        reg_count: usize,
        h_mix: *const u32,
    ) -> *const c_char;
    pub fn r0hip_poly_divide(d_poly: *mut u32, size: usize, h_remainder: *mut u32, h_z: *const u32) -> *const c_char;
    pub fn r0hip_combos_divide(
        d_combos: *mut u32,
        nchunks: usize,
        h_pows: *const u32,
        h_begin: *const u32,
        cycles: usize,
        bad_chunk: *mut i64,
    ) -> *const c_char;

    // ---- element-wise ----
    pub fn r0hip_eltwise_add_elem(d_out: *mut u32, d_a: *const u32, d_b: *const u32, count: usize) -> *const c_char;
    pub fn r0hip_eltwise_copy_elem(d_out: *mut u32, d_in: *const u32, count: usize) -> *const c_char;
    pub fn r0hip_eltwise_zeroize_elem(d_io: *mut u32, count: usize) -> *const c_char;
    pub fn r0hip_eltwise_sum_extelem(d_out: *mut u32, d_in: *const u32, to_add: usize, count: usize) -> *const c_char;
    pub fn r0hip_eltwise_copy_elem_slice(
        d_into: *mut u32,
        d_from: *const u32,
        from_rows: usize,
        from_cols: usize,
        from_offset: usize,
        from_stride: usize,
        into_offset: usize,
        into_stride: usize,
    ) -> *const c_char;
    pub fn r0hip_gather_sample(d_dst: *mut u32, d_src: *const u32, idx: usize, size: usize, stride: usize)
        -> *const c_char;
    pub fn r0hip_gather_sample_host(h_dst: *mut u32, d_src: *const u32, idx: usize, size: usize, stride: usize)
        -> *const c_char;
    /// the nodes MerkleTreeProver::prove reads for each opening j = h_idx[i] (merkle.rs:108-140):
    /// nodes[j], then nodes[(j >> k) ^ 1] for k < levels, straight to the host in one call
    pub fn r0hip_merkle_paths_host(
        h_dst: *mut u32,
        d_nodes: *const u32,
        heap_digests: usize,
        h_idx: *const u64,
        n: usize,
        levels: usize,
    ) -> *const c_char;
    pub fn r0hip_scatter(
        d_into: *mut u32,
        d_index: *const u32,
        d_offsets: *const u32,
        d_values: *const u32,
        cycles: usize,
    ) -> *const c_char;
    pub fn r0hip_prefix_products(d_io: *mut u32, count: usize) -> *const c_char;
    pub fn r0hip_fill_uniform(d_out: *mut u32, count: usize, seed: u64) -> *const c_char;
    /// keyed noise words: the ChaCha20 stream of (h_key, h_nonce) as field elements
    pub fn r0hip_fill_chacha20(d_out: *mut u32, count: usize, h_key: *const u32, h_nonce: *const u32) -> *const c_char;

    // ---- hashing (sppark_poseidon2_*, risc0_zkp_cuda_sha_*, sppark_poseidon254_*) ----
    pub fn r0hip_hash_rows(suite: c_int, d_out: *mut u32, d_matrix: *const u32, rows: usize, cols: usize)
        -> *const c_char;
    pub fn r0hip_hash_fold(suite: c_int, d_io: *mut u32, input_size: usize, output_size: usize) -> *const c_char;
    pub fn r0hip_merkle_tree(suite: c_int, d_nodes: *mut u32, d_matrix: *const u32, rows: usize, cols: usize)
        -> *const c_char;

    // ---- circuits ----
    pub fn r0hip_eval_check(
        circuit: *const c_char,
        d_check: *mut u32,
        d_groups: *const *const u32,
        d_mix: *const u32,
        d_global: *const u32,
        h_poly_mix: *const u32,
        po2: u32,
    ) -> *const c_char;
    pub fn r0hip_rv32im_accum_finalize(d_accum: *mut u32, rows: usize, cols: usize, last_cycle: usize)
        -> *const c_char;
    pub fn r0hip_rv32im_accum(
        d_data: *const u32,
        d_accum: *mut u32,
        d_global: *const u32,
        d_mix: *const u32,
        rows: usize,
        cols: usize,
        last_cycle: usize,
    ) -> *const c_char;
    pub fn r0hip_recursion_accum(
        d_ctrl: *const u32,
        d_global: *const u32,
        d_data: *const u32,
        d_mix: *const u32,
        d_accum: *mut u32,
        work_cycles: usize,
        total_cycles: usize,
    ) -> *const c_char;

    // ---- whole segments ----
    pub fn r0hip_prove_segment(
        circuit: *const c_char,
        suite: c_int,
        po2: u32,
        d_code: *const u32,
        d_data: *const u32,
        d_accum: *const u32,
        d_global: *mut u32,
        write_version: c_int,
        version: u32,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// prove_core with WitnessGenerator::accum inside (accum group given as witgen allocated it)
    pub fn r0hip_prove_segment_accum(
        circuit: *const c_char,
        suite: c_int,
        po2: u32,
        d_code: *const u32,
        d_data: *const u32,
        d_accum: *mut u32,
        work_cycles: usize,
        h_bigint: *const R0HipBigIntBack,
        n_bigint: usize,
        d_global: *mut u32,
        write_version: c_int,
        version: u32,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// WitnessGenerator::accum's BigInt state injection (witgen/mod.rs:178-205)
    pub fn r0hip_rv32im_bigint_accum_states(
        h_mix: *const u32,
        h_backs: *const R0HipBigIntBack,
        n: usize,
        rows: usize,
        h_states: *mut u32,
    ) -> *const c_char;
    /// the same states computed on the device into d_states (n x 12 words), complete on return
    pub fn r0hip_rv32im_bigint_accum_states_device(
        d_states: *mut u32,
        h_mix: *const u32,
        h_backs: *const R0HipBigIntBack,
        n: usize,
        rows: usize,
    ) -> *const c_char;
    pub fn r0hip_rv32im_bigint_accum_inject(
        d_accum: *mut u32,
        rows: usize,
        h_mix: *const u32,
        h_backs: *const R0HipBigIntBack,
        n: usize,
    ) -> *const c_char;
    /// risc0_circuit_rv32im_cuda_witgen's role (rv32im-sys ffi.cu:431-472): `buffers` and
    /// `preflight` point at risc0_circuit_rv32im_sys::{RawExecBuffers, RawPreflightTrace}
    /// (identical repr(C) layouts: struct r0hip_raw_exec_buffers / r0hip_raw_preflight_trace)
    pub fn r0hip_rv32im_witgen(
        mode: u32,
        buffers: *const c_void,
        preflight: *const c_void,
        cycles: u32,
    ) -> *const c_char;
    /// rv32im SegmentProverImpl::prove_core from a preflight trace (prove/hal/mod.rs:143-224)
    pub fn r0hip_prove_segment_trace(
        suite: c_int,
        po2: u32,
        mode: u32,
        h_global: *const u32,
        h_inj_index: *const u32,
        inj_rows: usize,
        h_inj_offsets: *const u32,
        h_inj_values: *const u32,
        preflight: *const c_void,
        h_bigint: *const R0HipBigIntBack,
        n_bigint: usize,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// build_injector plus hal.scatter from the Back records, in front of r0hip_rv32im_witgen
    pub fn r0hip_rv32im_inject_backs(
        d_data: *mut u32,
        rows: usize,
        h_cycles: *const c_void,
        backs: *const R0HipBacks,
    ) -> *const c_char;
    /// r0hip_prove_segment_trace from the Back records: no injector arrays, no BigInt records
    pub fn r0hip_prove_segment_trace_backs(
        suite: c_int,
        po2: u32,
        mode: u32,
        h_global: *const u32,
        preflight: *const c_void,
        backs: *const R0HipBacks,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// r0hip_prove_segment_trace with every input resident on the device
    pub fn r0hip_prove_segment_trace_resident(
        suite: c_int,
        po2: u32,
        mode: u32,
        d_global: *const u32,
        d_inj_index: *const u32,
        inj_rows: usize,
        d_inj_offsets: *const u32,
        d_inj_values: *const u32,
        d_preflight: *const c_void,
        h_bigint: *const R0HipBigIntBack,
        n_bigint: usize,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// risc0_circuit_recursion_cuda_witgen's role (recursion-sys ffi.cpp:191-205)
    pub fn r0hip_recursion_witgen(
        d_ctrl: *const u32,
        d_data: *mut u32,
        d_global: *mut u32,
        total_cycles: usize,
        h_wom: *const u32,
        n_wom: usize,
        h_cycles: *const u32,
        n_cycles: usize,
        h_iops: *const u32,
        n_iops: usize,
    ) -> *const c_char;
    /// RecursionProverImpl::prove from the program and its preflight (recursion prove/mod.rs:160-230)
    pub fn r0hip_prove_recursion(
        suite: c_int,
        po2: u32,
        d_ctrl: *const u32,
        h_wom: *const u32,
        n_wom: usize,
        h_cycles: *const u32,
        n_cycles: usize,
        h_iops: *const u32,
        n_iops: usize,
        noise_seed: u64,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// the same with the ZK noise from a keyed ChaCha20 stream (h_key NULL: an OS key): the one to ship
    pub fn r0hip_prove_recursion_keyed(
        suite: c_int,
        po2: u32,
        d_ctrl: *const u32,
        h_wom: *const u32,
        n_wom: usize,
        h_cycles: *const u32,
        n_cycles: usize,
        h_iops: *const u32,
        n_iops: usize,
        h_key: *const u32,
        stream_id: u64,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    // ---- resident recursion programs (program.rs:33-104, witgen.rs:57-67) ----
    /// the control group and its commitment from Program.code, made once (h_code: 23 words per row)
    pub fn r0hip_recursion_program_create(
        out: *mut *mut R0HipRecursionProgram,
        suite: c_int,
        po2: u32,
        h_code: *const u32,
        n_words: usize,
        form: c_int,
    ) -> *const c_char;
    /// every out pointer may be null; control_id is Program::compute_control_id's digest
    pub fn r0hip_recursion_program_info(
        program: *const R0HipRecursionProgram,
        suite: *mut c_int,
        po2: *mut u32,
        code_rows: *mut usize,
        control_id: *mut u32,
        device_bytes: *mut u64,
    ) -> *const c_char;
    pub fn r0hip_recursion_program_ctrl(program: *const R0HipRecursionProgram, d_ctrl: *mut *const u32) -> *const c_char;
    /// r0hip_prove_recursion_keyed's seal with the control group's commitment taken from the handle
    pub fn r0hip_prove_recursion_program(
        program: *const R0HipRecursionProgram,
        h_wom: *const u32,
        n_wom: usize,
        h_cycles: *const u32,
        n_cycles: usize,
        h_iops: *const u32,
        n_iops: usize,
        h_key: *const u32,
        stream_id: u64,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    /// refused (nothing freed) while a proof or a queued worker job uses the handle
    pub fn r0hip_recursion_program_destroy(program: *mut R0HipRecursionProgram) -> *const c_char;
    /// The native preflight (Preflight::step, prove/preflight.rs:181-627) of a program's words on
    /// `input`; all four out arrays null: the size query. Host only.
    pub fn r0hip_recursion_preflight(
        h_code: *const u32,
        n_words: usize,
        form: c_int,
        po2: u32,
        h_input: *const u32,
        n_input: usize,
        h_wom: *mut u32,
        wom_cap: usize,
        n_wom: *mut usize,
        h_cycles: *mut u32,
        cycles_cap: usize,
        n_cycles: *mut usize,
        h_iops: *mut u32,
        iops_cap: usize,
        n_iops: *mut usize,
        h_output: *mut u32,
        output_cap: usize,
        n_output: *mut usize,
    ) -> *const c_char;
    pub fn r0hip_recursion_program_prepare_input(program: *const R0HipRecursionProgram) -> *const c_char;
    pub fn r0hip_recursion_last_preflight_ms(out: *mut f64) -> *const c_char;
    pub fn r0hip_recursion_program_input_info(
        program: *const R0HipRecursionProgram,
        out: *mut R0HipRecursionInputInfo,
    ) -> *const c_char;
    /// RecursionProver::prove(program, input) from a handle: preflight, planned witness generation,
    /// r0hip_prove_recursion_program's sequence
    pub fn r0hip_prove_recursion_program_input(
        program: *const R0HipRecursionProgram,
        h_input: *const u32,
        n_input: usize,
        h_key: *const u32,
        stream_id: u64,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
        h_output: *mut u32,
        output_cap: usize,
        n_output: *mut usize,
    ) -> *const c_char;
    pub fn r0hip_prove_segments(
        circuit: *const c_char,
        suite: c_int,
        po2: u32,
        write_version: c_int,
        version: u32,
        jobs: *mut R0HipSegmentJob,
        njobs: usize,
        in_flight: u32,
    ) -> *const c_char;
    pub fn r0hip_prove_trace_segments(
        suite: c_int,
        po2: u32,
        jobs: *mut R0HipTraceJob,
        njobs: usize,
        in_flight: u32,
        verify: c_int,
    ) -> *const c_char;

    // ---- the GPU worker: a persistent queue of rv32im and recursion jobs ----
    pub fn r0hip_worker_create(
        out: *mut *mut R0HipWorker,
        max_po2: u32,
        in_flight: u32,
        verify: c_int,
        h_noise_key: *const u32,
    ) -> *const c_char;
    pub fn r0hip_worker_submit(w: *mut R0HipWorker, job: *mut R0HipWorkerJob) -> *const c_char;
    pub fn r0hip_worker_wait(w: *mut R0HipWorker, done: *mut *mut R0HipWorkerJob, timeout_ms: i64) -> *const c_char;
    pub fn r0hip_worker_destroy(w: *mut R0HipWorker) -> *const c_char;
    // the witness check for the jobs submitted from now on (recorded at submit)
    pub fn r0hip_worker_set_witness_check(w: *mut R0HipWorker, on: c_int) -> *const c_char;
    // kind-4 preflights on n pool threads (0..8; 0: on the uploader thread, the default); refused
    // while a job is outstanding. `was` may be null.
    pub fn r0hip_worker_set_preflight_threads(w: *mut R0HipWorker, n: u32, was: *mut u32) -> *const c_char;
    // out_size: size_of::<R0HipWorkerStats>()
    pub fn r0hip_worker_get_stats(w: *mut R0HipWorker, out: *mut R0HipWorkerStats, out_size: usize) -> *const c_char;

    // ---- verification (host-only) ----
    pub fn r0hip_verify_seal(
        circuit: *const c_char,
        suite: c_int,
        seal: *const u32,
        seal_len: usize,
        h_code_roots: *const u32,
        n_code_roots: usize,
        h_code_root_out: *mut u32,
        po2_out: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_testing_verify_seal_structure(
        circuit: *const c_char,
        suite: c_int,
        seal: *const u32,
        seal_len: usize,
        po2_out: *mut u32,
    ) -> *const c_char;
    // ---- verification with the Merkle openings on the device (opt-in; `where_` is the C `where`) ----
    pub fn r0hip_verify_seal_on(
        where_: c_int,
        circuit: *const c_char,
        suite: c_int,
        seal: *const u32,
        seal_len: usize,
        h_code_roots: *const u32,
        n_code_roots: usize,
        h_code_root_out: *mut u32,
        po2_out: *mut u32,
    ) -> *const c_char;
    // process-wide, 0 by default: Poseidon254 openings of a device check on the device too
    pub fn r0hip_set_verify_device_poseidon254(on: c_int) -> *const c_char;
    pub fn r0hip_testing_verify_seal_structure_on(
        where_: c_int,
        circuit: *const c_char,
        suite: c_int,
        seal: *const u32,
        seal_len: usize,
        po2_out: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_merkle_open_digests(
        suite: c_int,
        h_words: *const u32,
        n_words: usize,
        h_open: *const R0HipOpening,
        n_open: usize,
        h_digests: *mut u32,
        h_status: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_poly_ext(
        circuit: *const c_char,
        h_mix: *const u32,
        h_global: *const u32,
        h_eval_u: *const u32,
        h_poly_mix: *const u32,
        h_out: *mut u32,
    ) -> *const c_char;
    // the constraint polynomial on the 2^po2 trace rows of the witness groups (a diagnostic):
    // d_out (may be null) gets one FpExt per row, the report names the rows that are nonzero
    pub fn r0hip_constraint_rows(
        circuit: *const c_char,
        po2: u32,
        d_code: *const u32,
        d_data: *const u32,
        d_accum: *const u32,
        d_mix: *const u32,
        d_global: *const u32,
        h_poly_mix: *const u32,
        d_out: *mut u32,
        report: *mut R0HipConstraintReport,
    ) -> *const c_char;
    // host-only: the id in <circuit>.poly.ir of the first term one row's taps violate (-1: none)
    pub fn r0hip_constraint_term(
        circuit: *const c_char,
        h_taps: *const u32,
        h_mix: *const u32,
        h_global: *const u32,
        h_poly_mix: *const u32,
        term: *mut i32,
    ) -> *const c_char;

    // ---- circuits compiled in, accumulation by callback, the demo circuit, the self-test ----
    pub fn r0hip_circuit_info(
        circuit: *const c_char,
        out: *mut R0HipCircuitDesc,
        out_size: usize,
        names: *mut c_char,
        names_cap: usize,
    ) -> *const c_char;
    // host-only: a circuit registered at run time (interpreted eval_check), and the testing-only
    // points per interpreter launch
    pub fn r0hip_circuit_register(t: *const R0HipCircuitTables, t_size: usize) -> *const c_char;
    pub fn r0hip_testing_set_interp_chunk(points: u32, was: *mut u32) -> *const c_char;
    // host-only: a circuit module (the circuit's generated kernels as a shared object of their
    // own, include/r0hip_module.h) loaded at run time; loading runs its code, as linking it would.
    // name_out (may be null) takes the circuit's name, name_cap >= 32. kind: 0 compiled in,
    // 1 registered (interpreted), 2 a module.
    pub fn r0hip_circuit_load(path: *const c_char, name_out: *mut c_char, name_cap: usize) -> *const c_char;
    pub fn r0hip_circuit_backend(circuit: *const c_char, kind: *mut c_int) -> *const c_char;
    pub fn r0hip_prove_segment_cb(
        circuit: *const c_char,
        suite: c_int,
        po2: u32,
        d_code: *const u32,
        d_data: *const u32,
        accum: R0HipAccumFn,
        user: *mut c_void,
        d_global: *mut u32,
        write_version: c_int,
        version: u32,
        h_seal: *mut u32,
        seal_cap: usize,
        seal_len: *mut usize,
        h_mix_out: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_demo_witness(
        po2: u32,
        n_active: usize,
        a0: u32,
        b0: u32,
        d_code: *mut u32,
        d_data: *mut u32,
        d_global: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_demo_accum(
        po2: u32,
        n_active: usize,
        d_data: *const u32,
        h_mix: *const u32,
        d_accum: *mut u32,
    ) -> *const c_char;
    pub fn r0hip_selftest(
        suites_mask: u32,
        po2: u32,
        out: *mut R0HipSelftestReport,
        out_size: usize,
    ) -> *const c_char;

    // ---- diagnostics (scope! spans and the MemoryTracker) ----
    pub fn r0hip_set_kernel_timing(on: c_int) -> *const c_char;
    pub fn r0hip_kernel_times(buf: *mut c_char, cap: usize) -> *const c_char;
    pub fn r0hip_last_profile(buf: *mut c_char, cap: usize) -> *const c_char;
    pub fn r0hip_mem_stats(out: *mut u64) -> *const c_char;
    pub fn r0hip_mem_reset_peak() -> *const c_char;
    pub fn r0hip_trim() -> *const c_char;
}
