// Circuit modules (include/r0hip_module.h, r0hip_circuit_load): the host checks a descriptor
// passes before its circuit enters the registry, so that a stale or mismatched module is a
// refusal that names what disagrees and never out-of-range device addressing.
//   check_descriptor   the ABI number, the three struct sizes, the architecture, the pointers
//   rt::validate       the tables, as r0hip_circuit_register checks them (circuit_rt.h)
//   check_kernel_view  what info() / rows_info() say the kernels index, against the tables
// Plain C++17 with no HIP header, so the same source builds into a stand-alone host program
// (tests/circuit_module_check.cpp, under a sanitizer).
#pragma once
#include <string>

#include "../../include/r0hip_module.h"
#include "evalcheck_types.h"

namespace r0 {
namespace mod {

// limits the driver sizes its tables and scratch by (prover.cpp ec_tables; the generator's
// `wide` mask has one bit per kernel)
constexpr int kMaxKernels = 64;
constexpr int kMaxMat = 1 << 16;      // materialised values of one type
constexpr int kMaxCombos = 1 << 16;   // folded products
constexpr int kMaxComboLen = 1 << 8;  // powers of one folded product
constexpr int kMaxCols = 1 << 20;
constexpr int kMaxUniform = 1 << 20;

// The library's view of the three sizes and of its architecture
struct Expect {
  uint32_t desc_size, args_size, info_size;
  const char* arch;
};
inline Expect expect_here(const char* arch) {
  return Expect{uint32_t(sizeof(r0hip_module_desc)), uint32_t(sizeof(EvalCheckArgs)), uint32_t(sizeof(EvalCheckInfo)),
                arch};
}

using InfoFn = void (*)(EvalCheckInfo*);

// Each returns "" or the refusal, without the path.
std::string check_descriptor(const r0hip_module_desc* d, const Expect& want);
// family: "info" (eval_check's) or "rows_info"
std::string check_kernel_view(const r0hip_circuit_tables& t, const EvalCheckInfo& info, const char* family);
// All three stages in load order; calls the descriptor's info() and rows_info().
std::string check_module(const r0hip_module_desc* d, const Expect& want);

}  // namespace mod
}  // namespace r0
