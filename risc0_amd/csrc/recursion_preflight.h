// The recursion circuit's preflight on the host: Preflight::step and its ops
// (risc0/circuit/recursion/src/prove/preflight.rs:181-627) over bb31.h arithmetic, so a proof
// can start from a program and the words the reference calls `input`
// (RecursionProver::prove, prove/mod.rs:165). Host-only: plain C++17, no HIP.
//
// A program is decoded once into an op table (decode); a run reads 12 words per row from it
// instead of 23 field words, and everything that depends on the program alone comes out of the
// decoding: each cycle's {iopIdx, isParSafe}, the final size of the write-once memory (every
// write address is in the code), the number of IOP values and of output words, and the number
// of input words the READ_IOP_HEADER ops consume.
//
// The library's limit: a WOM address at or above 16 * 2^po2 cells is refused (the reference
// grows its vector to any address below p). The witness generator allows at most 9 WOM
// argument rows per cycle, so a program it accepts stays below the cap, and malformed code can
// not ask for gigabytes.
//
// Not run: checked_bytes rows (the C++ witness generators throw in extern_readCoefficients);
// decode refuses them, naming the row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace r0 {
namespace rpf {

constexpr uint32_t kCodeCols = 23;
constexpr uint32_t kZkCycles = 1024;

// selector kinds (CODE_LAYOUT.code.select, checked in Preflight::step's order)
enum Kind : uint8_t { kIllegal = 0, kMacro, kMicro, kP2Load, kP2Full, kP2Partial, kP2Store };
// macro sub-ops that the preflight distinguishes (macro_op's order); everything else is a nop
enum MacroOp : uint8_t { kMacroNop = 0, kBitAndElem, kBitOpShorts, kShaInit, kShaLoad, kShaMix, kShaFini };
// micro opcodes (preflight.rs:41-53); kUnknown for any other word
enum MicroOp : uint8_t {
  kConst = 0, kAdd, kSub, kMul, kInv, kEq, kReadIopHeader, kReadIopBody, kMixRng, kSelect, kExtract,
  kUnknown = 0xFF
};
// p2_load / p2_store flags
constexpr uint8_t kFlagDoMont = 1, kFlagKeepState = 2, kFlagKeepUpper = 4;

// One program row. arg holds plain integers below p.
//   micro:    sub[i] the opcode of op i, arg[3i .. 3i+2] its operands
//   macro:    sub[0] the MacroOp, arg[0..2] the operands; sub[1] for the SHA ops their position in
//             the group, which the row order fixes (sha_init and sha_fini: 0..3, sha_load: 0..15)
//   p2_load:  sub[0] flags, sub[1] the group (0..2, 0xFF out of range), arg[0..7] the input addresses
//   p2_store: sub[0] flags, sub[1] the group
struct Op {
  uint8_t kind;
  uint8_t sub[3];
  uint32_t wa;  // write_addr
  uint32_t arg[9];
};

struct Program {
  uint32_t po2 = 0;
  std::vector<Op> ops;           // one per program row
  std::vector<uint32_t> cycles;  // RawPreflightCycle {iop_idx, is_par_safe} per row
  size_t n_wom = 0;              // cells of the WOM after a complete run
  size_t n_iops = 0;             // READ_IOP_BODY ops
  size_t n_output = 0;           // ADD ops with a[2] != 0
  uint64_t n_input = 0;          // input words the READ_IOP_HEADER ops consume
  size_t wom_cap() const { return size_t(16) << po2; }
};

// code: 23 words per row, row-major; form 0 plain words of a .zkr (reduced mod p as Elem::from
// does), form 1 canonical Montgomery words. Throws std::runtime_error on a malformed argument or a
// checked_bytes row.
Program decode(const uint32_t* code, size_t n_words, int form, uint32_t po2);
// the same from the control group on the host: 23 columns of n = 2^po2 Montgomery words
Program decode_columns(const uint32_t* ctrl, size_t rows, uint32_t po2);

// One run. wom (4 * n_wom words), iops (4 * n_iops) and output (n_output) are the caller's, and
// any of them may be page-locked staging memory: wom is zeroed first, then written in place as
// Montgomery words; output holds plain integers. Throws std::runtime_error with the reference's
// message where it has one, followed by " (cycle N)".
void run(const Program& p, const uint32_t* input, size_t n_input, uint32_t* wom, uint32_t* iops, uint32_t* output);

}  // namespace rpf
}  // namespace r0
