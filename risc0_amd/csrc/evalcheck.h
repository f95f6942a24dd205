// Interface between the host driver and the generated per-circuit eval_check and
// constraint-rows kernels (risc0_amd/csrc/gen/<circuit>/eval_check_<circuit>.hip and
// rows_<circuit>.hip, emitted at build time by tools/gen_eval_check.py from
// risc0_amd/circuits/<circuit>.poly.ir).
// The two structs are in evalcheck_types.h, which needs no HIP header.
#pragma once
#include "evalcheck_types.h"
#include "runtime.h"

namespace r0 {

void eval_check_rv32im(hipStream_t s, const EvalCheckArgs& e);
void eval_check_rv32im_info(EvalCheckInfo* info);
void eval_check_recursion(hipStream_t s, const EvalCheckArgs& e);
void eval_check_recursion_info(EvalCheckInfo* info);

// The constraint-rows family (gen/<circuit>/rows_<circuit>*.hip, the generator's second output
// from the same program): poly_fp on the N = e.domain trace rows themselves, zero exactly on the
// rows that satisfy every constraint. The witness groups are read as they are, a tap at
// (row - back) & (N - 1), so args and colptr address N-row columns. The result is one FpExt per
// row, AoS, in e.acc (N x 4 words); e.check and e.vinv are not read. The info is the family's
// own (its poly_mix table, scratch sizes and lane-independent values differ from eval_check's).
void constraint_rows_rv32im(hipStream_t s, const EvalCheckArgs& e);
void constraint_rows_rv32im_info(EvalCheckInfo* info);
void constraint_rows_recursion(hipStream_t s, const EvalCheckArgs& e);
void constraint_rows_recursion_info(EvalCheckInfo* info);

}  // namespace r0
