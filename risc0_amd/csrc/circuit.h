// Circuit descriptions compiled into the library: the TapSet
// (risc0/zkp/src/taps.rs:57-66), CircuitInfo (adapter.rs:122-126), the order of the
// eval_check argument buffers, and the generated eval_check entry points.
// The tables come from risc0_amd/circuits/*.taps.json via tools/gen_circuits_inc.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "evalcheck.h"

namespace r0 {

namespace rt {
struct Programs;  // circuit_rt.h
}

struct CircuitDef {
  const char* name;
  const uint32_t* taps;  // n_taps x {offset, back, group, combo, skip}
  size_t n_taps;
  const uint32_t* combo_taps;
  size_t n_combo_taps;
  const uint32_t* combo_begin;  // combos_count + 1
  size_t combos_count;
  const uint32_t* group_begin;  // n_groups + 1
  size_t n_groups;
  const uint32_t* group_sizes;
  const uint32_t* poly_mix_powers;
  size_t n_poly_mix;
  const char* circuit_info;  // 16 bytes
  size_t mix_size, output_size;
  const int* eval_args;  // >= 0 register group, -1 mix, -2 out (global)
  size_t n_eval_args;
  void (*eval_check)(hipStream_t, const EvalCheckArgs&);
  void (*info)(EvalCheckInfo*);
  // the same program on the trace rows (evalcheck.h: the constraint-rows family)
  void (*constraint_rows)(hipStream_t, const EvalCheckArgs&);
  void (*rows_info)(EvalCheckInfo*);
  // the constraint program for the host poly_ext (verify.cpp): n_ir records of
  // {op, dst, a, b, c, d}, op index into "celg+-*abr", dst dense 0..n_ir-1
  const uint32_t* ir;
  size_t n_ir;
  // A circuit registered at run time (r0hip_circuit_register, circuit_registry.cpp): the four
  // kernel pointers above are null and the device interprets these programs (eval_interp.hip).
  // Null for every compiled-in circuit, and null for a circuit loaded from a circuit module
  // (r0hip_circuit_load): that one is a run-time entry too, but its four kernel pointers are the
  // module's generated kernels and every table above points into the module, which stays open.
  // So `interp` alone decides between the interpreter and the generated kernels.
  const rt::Programs* interp = nullptr;

  struct Tap {
    uint32_t offset, back, group, combo, skip;
  };
  const Tap& tap(size_t i) const { return reinterpret_cast<const Tap*>(taps)[i]; }
  size_t group_size(size_t g) const { return tap(group_begin[g + 1] - 1).offset + 1; }
  // RegisterIter (taps.rs:202-227): calls f(first tap index of each register)
  template <typename F>
  void regs(size_t begin, size_t end, F f) const {
    size_t cur = begin;
    while (cur < n_taps) {
      size_t next = cur + tap(cur).skip;
      if (next > end) break;
      f(cur);
      cur = next;
    }
  }
};

// The circuits compiled in, in build order (tools/circuit_files.py: the shipped ones, the demo
// circuit, then those plugged in with EXTRA_CIRCUIT_DIRS). gen/circuits.cpp defines these three;
// the generator writes them as find_circuit, circuit_count and circuit_at, as it did before there
// was a registry, and Makefile.objs renames them for that one file.
const CircuitDef* compiled_find_circuit(const std::string& name);
size_t compiled_circuit_count();
const CircuitDef& compiled_circuit_at(size_t i);

// Every circuit the process knows (circuit_registry.cpp): the compiled-in ones, then the
// run-time entries in the order they arrived, whether registered from tables
// (r0hip_circuit_register, interpreted) or loaded from a circuit module (r0hip_circuit_load, its
// own generated kernels); both kinds share the kMaxRegistered entries. Readers take no lock: the registry is an
// append-only table of kMaxRegistered entries behind an atomic count, and an entry never moves
// or goes away.
constexpr size_t kMaxRegistered = 64;
const CircuitDef* find_circuit(const std::string& name);
size_t circuit_count();
const CircuitDef& circuit_at(size_t i);
// "unknown circuit X (compiled in: a, b, c)", and once there is a run-time entry
// "unknown circuit X (compiled in: a, b, c; registered: d)": loaded names stand among the
// registered ones under the same word
std::string unknown_circuit(const char* name);
// r0hip_circuit_backend: 0 compiled in, 1 registered (interpreted), 2 a module, -1 unknown
int circuit_backend(const std::string& name);

}  // namespace r0
