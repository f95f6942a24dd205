// What the plug-in circuits add to the prover: the accumulation by callback
// (r0hip_prove_segment_cb) and the demo circuit's device side (demo_circuit.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace r0 {

// prove_segment with the accum group made after the mix is drawn: the prover allocates the group
// (INVALID words), drains its stream and calls fn on the proving thread with the mix on the
// host. fn may queue work on `stream` or write the group with synchronous copies of its own. It
// returns NULL, or a message that fails the proof (the string stays the callback's).
struct AccumCallback {
  const char* (*fn)(void* user, const uint32_t* h_mix, uint32_t* d_accum, void* stream);
  void* user;
};

// The demo circuit (risc0_amd/circuits/demo.*, tools/gen_demo_circuit.py). Groups are
// column-major, rows = 2^po2, 1 <= n <= rows active rows; a0, b0 are Montgomery words.
//   demo_witness: code (3 columns, every row), data (3 columns, rows < n only: the rows above
//                 are the caller's, e.g. ZK noise) and the 3 global words
//   demo_accum  : accum (4 columns, rows < n only) from data column a and the 4 mix words
void demo_witness(hipStream_t s, uint32_t po2, size_t n, uint32_t a0, uint32_t b0, uint32_t* code, uint32_t* data,
                  uint32_t* global);
void demo_accum(hipStream_t s, uint32_t po2, size_t n, const uint32_t* data, const uint32_t* h_mix, uint32_t* accum);

}  // namespace r0
