// Circuits registered at run time (r0hip_circuit_register): the host half that needs no HIP.
//   validate   everything the device interpreter's addressing rests on, restated from
//              tools/circuit_files.py validate(); a refusal names the field
//   compile    the constraint program (CircuitDef::ir) into the bytecode eval_interp.hip runs
// Plain C++17 with no HIP header, so the same source builds into a stand-alone host program
// (tests/circuit_rt_check.cpp, under a sanitizer).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/r0hip.h"

namespace r0 {
namespace rt {

constexpr size_t kMaxIr = size_t(1) << 20;   // records of one constraint program
constexpr size_t kMaxWords = size_t(1) << 24;  // mix_size, output_size (a `g` operand's index field)
constexpr size_t kMaxEvalArgs = 16;
constexpr size_t kMaxName = 31;

// The constraint program's op codes, the index into "celg+-*abr" (CircuitDef::ir)
enum IrOp : uint32_t { IR_C, IR_E, IR_L, IR_G, IR_ADD, IR_SUB, IR_MUL, IR_A, IR_B, IR_R };

// ---- the bytecode ----
// One record per `+ - * a b` of the program, in program order, then one RET. The values of
// `c e l g` records get no record and no slot: an operand that names one is read where it is
// used. An operand is a kind and a value:
enum OperandKind : uint32_t {
  K_NONE = 0,
  K_FP_SLOT,   // value = Fp slot
  K_EXT_SLOT,  // value = FpExt slot
  K_FP_IMM,    // value = the Montgomery word (c)
  K_EXT_IMM,   // value = index into Programs::consts, 4 words each (e)
  K_WORD,      // value = (eval_args index << 24) | word index: mix or global (g)
  K_TAP,       // value = tap index (l): Programs::taps_check / taps_rows
};
constexpr bool kind_is_ext(uint32_t k) { return k == K_EXT_SLOT || k == K_EXT_IMM; }

// The opcode carries the operand types: base * 4 + (first operand is FpExt) + 2 * (second is).
// ACC_A: dst = acc + x * pow[k] (first = x, second unused); ACC_B: dst = acc + x * y * pow[k]
// (first = x, second = y). The accumulator is always FpExt and so is their result; ADD/SUB/MUL
// give the wider operand's type; RET hands the first operand to the kernel's epilogue.
enum Base : uint32_t { B_ADD = 0, B_SUB = 1, B_MUL = 2, B_ACC_A = 3, B_ACC_B = 4, B_RET = 5 };

// 8 words, read by every lane of a wave at the same address
struct Record {
  uint32_t op;     // Base * 4 + type bits
  uint32_t dst;    // slot, in the file the result's type names
  uint32_t kinds;  // operand kinds: x | y << 4 | acc << 8
  uint32_t x, y, acc;  // operand values
  uint32_t k;      // poly_mix power (ACC_A, ACC_B)
  uint32_t pad;
};
static_assert(sizeof(Record) == 32, "the kernel reads records as 8 words");

// A tap as the kernel reads it: args[arg][col * n + ((i - back) & (n - 1))]
struct TapRef {
  uint32_t arg, col, back, pad;
};

// Both programs of a circuit. They differ only in the tap stride (eval_check reads a tap 4 * back
// points behind on the 4N domain, the rows family back rows behind), so they share the records
// and carry a tap table each.
struct Programs {
  std::vector<Record> code;
  std::vector<uint32_t> consts;  // 4 words per K_EXT_IMM
  std::vector<TapRef> taps_check, taps_rows;
  uint32_t n_fp_slots = 0, n_ext_slots = 0;
  double modmuls = 0;  // field multiplications per point (Fp x Fp 1, Fp x FpExt 4, FpExt x FpExt 16)
  size_t slot_words() const { return size_t(n_fp_slots) + 4 * size_t(n_ext_slots); }
};

// "" when the tables are sound, else "<field>: <why>". The name's uniqueness is the registry's.
std::string validate(const r0hip_circuit_tables& t);
// Type of every value of a validated program: 0 Fp, 1 FpExt, indexed by id.
std::vector<uint8_t> infer_types(const uint32_t* ir, size_t n_ir);
// The bytecode of validated tables.
Programs compile(const r0hip_circuit_tables& t);

}  // namespace rt
}  // namespace r0
