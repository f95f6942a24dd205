"""risc0_amd — MI355X-native STARK prover backend for risc0-zkp.

The product is libr0hip.so (risc0_amd/lib, built from risc0_amd/csrc by
__graft_entry__.build()): hand-written HIP kernels for gfx950 behind the C ABI
in include/r0hip.h, plus a C++ segment prover. This package is a thin ctypes
mirror of the reference's `Hal` trait for tests and the benchmark.
"""
from .hal import (POSEIDON2, POSEIDON254, SHA256, BigIntBack, Buffer, HipHal, R0HipError, bigint_accum_inject,
                  bigint_accum_states, bigint_accum_states_device, bigint_backs, BIGINT_BACK_DTYPE, check, prove_recursion, recursion_witgen, rv32im_witgen, prove_segment_trace, ResidentTrace,
                  prove_segment_trace_resident, exported_symbols, kernel_times,
                  last_profile, lib, mem_reset_peak, mem_stats, trim, prove_segment, prove_segment_accum, prove_segments,
                  set_kernel_timing, poly_ext, verify_seal, TraceJob, prove_trace_segments, host_array, pinned_copy,
                  fill_chacha20, prove_recursion_keyed, RecursionInput, WorkerJobStruct, Worker, call_stats,
                  set_proof_streams, Back, BacksStruct, Backs, BacksJob, BACK_WORDS, rv32im_inject_backs,
                  prove_segment_trace_backs, RecursionProgram, CODE_ENCODED, CODE_MONTGOMERY,
                  WorkerProgramJobStruct, WorkerInputJobStruct, WorkerStats, RecursionInputInfo, recursion_preflight,
                  recursion_last_preflight_ms, Opening, merkle_open_digests, set_verify_device_poseidon254,
                  VERIFY_RECEIPTS_DEVICE, ConstraintReport,
                  constraint_rows, constraint_term, set_witness_check, circuit_names, circuit_info,
                  prove_segment_cb, demo_witness, demo_accum, selftest, CircuitDesc, SelftestReport,
                  CircuitTables, circuit_tables_struct, register_circuit, testing_set_interp_chunk,
                  load_circuit_module, circuit_backend, build_circuit_module, MODULE_DIR)

__all__ = ["POSEIDON2", "POSEIDON254", "SHA256", "BigIntBack", "bigint_accum_inject", "bigint_accum_states", "bigint_accum_states_device", "bigint_backs", "BIGINT_BACK_DTYPE", "prove_recursion", "recursion_witgen", "rv32im_witgen", "prove_segment_trace", "ResidentTrace", "prove_segment_trace_resident", "Buffer", "HipHal", "R0HipError", "check", "exported_symbols", "last_profile",
           "lib", "mem_reset_peak", "mem_stats", "trim", "prove_segment", "prove_segment_accum", "prove_segments",
           "kernel_times", "set_kernel_timing", "poly_ext", "verify_seal", "TraceJob", "prove_trace_segments",
           "host_array", "pinned_copy", "fill_chacha20", "prove_recursion_keyed", "RecursionInput", "WorkerJobStruct",
           "Worker", "call_stats", "set_proof_streams", "Back", "BacksStruct", "Backs", "BacksJob", "BACK_WORDS",
           "rv32im_inject_backs", "prove_segment_trace_backs", "RecursionProgram", "CODE_ENCODED", "CODE_MONTGOMERY",
           "WorkerProgramJobStruct", "WorkerInputJobStruct", "WorkerStats", "RecursionInputInfo", "recursion_preflight",
           "recursion_last_preflight_ms", "Opening", "merkle_open_digests", "set_verify_device_poseidon254",
           "VERIFY_RECEIPTS_DEVICE",
           "ConstraintReport", "constraint_rows", "constraint_term", "set_witness_check", "circuit_names", "circuit_info",
           "prove_segment_cb", "demo_witness", "demo_accum", "selftest", "CircuitDesc", "SelftestReport",
           "CircuitTables", "circuit_tables_struct", "register_circuit", "testing_set_interp_chunk",
           "load_circuit_module", "circuit_backend", "build_circuit_module", "MODULE_DIR"]
