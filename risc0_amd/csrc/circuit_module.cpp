// Circuit modules: the descriptor and kernel-view checks of the load path (circuit_module.h).
// Host code only, no HIP header: it runs once per r0hip_circuit_load.
#include "circuit_module.h"

#include <string.h>

#include "circuit_rt.h"

namespace r0 {
namespace mod {
namespace {

std::string num(long long v) { return std::to_string(v); }

std::string differs(const char* field, const char* what, uint64_t module, uint64_t library) {
  return std::string(field) + ": the module has " + num(module) + what + ", the library " + num(library);
}

}  // namespace

std::string check_descriptor(const r0hip_module_desc* d, const Expect& want) {
  if (!d) return "the entry function returned no descriptor";
  // the ABI number is the first word of every descriptor there will ever be: read it alone first
  if (d->abi != R0HIP_MODULE_ABI) return differs("abi", " for R0HIP_MODULE_ABI", d->abi, R0HIP_MODULE_ABI);
  if (d->desc_size != want.desc_size)
    return differs("desc_size", " for sizeof(r0hip_module_desc)", d->desc_size, want.desc_size);
  if (d->args_size != want.args_size)
    return differs("args_size", " for sizeof(EvalCheckArgs)", d->args_size, want.args_size);
  if (d->info_size != want.info_size)
    return differs("info_size", " for sizeof(EvalCheckInfo)", d->info_size, want.info_size);
  if (!d->arch) return "arch: NULL";
  if (strnlen(d->arch, 64) == 64 || strcmp(d->arch, want.arch) != 0)
    return "arch: the module was compiled for " + std::string(d->arch, strnlen(d->arch, 64)) +
           ", the library for " + want.arch;
  if (!d->eval_check) return "eval_check: NULL";
  if (!d->info) return "info: NULL";
  if (!d->constraint_rows) return "constraint_rows: NULL";
  if (!d->rows_info) return "rows_info: NULL";
  return "";
}

std::string check_kernel_view(const r0hip_circuit_tables& t, const EvalCheckInfo& info, const char* family) {
  const std::string f = std::string(family) + "(): ";
  if (info.nargs < 0 || size_t(info.nargs) != t.n_eval_args)
    return f + "nargs: the kernels take " + num(info.nargs) + " arguments, eval_args has " + num((long long)t.n_eval_args);
  if (info.kernels < 1 || info.kernels > kMaxKernels)
    return f + "kernels: " + num(info.kernels) + " is not 1 to " + num(kMaxKernels);
  if (info.mat_fp < 0 || info.mat_fp > kMaxMat) return f + "mat_fp: " + num(info.mat_fp) + " is not 0 to " + num(kMaxMat);
  if (info.mat_ext < 0 || info.mat_ext > kMaxMat)
    return f + "mat_ext: " + num(info.mat_ext) + " is not 0 to " + num(kMaxMat);
  if (info.npm < 0 || size_t(info.npm) > t.n_poly_mix)
    return f + "npm: the kernels index " + num(info.npm) + " poly_mix powers, poly_mix_powers has " +
           num((long long)t.n_poly_mix);
  // the folded products: count, then that many indices into the powers
  if (info.ncombos < 0 || info.ncombos > kMaxCombos)
    return f + "ncombos: " + num(info.ncombos) + " is not 0 to " + num(kMaxCombos);
  if (info.ncombos && !info.combos) return f + "combos: NULL with ncombos " + num(info.ncombos);
  for (int j = 0, k = 0; j < info.ncombos; j++) {
    const int n = info.combos[k++];
    if (n < 1 || n > kMaxComboLen)
      return f + "combos: product " + num(j) + " has " + num(n) + " factors, not 1 to " + num(kMaxComboLen);
    for (int q = 0; q < n; q++, k++)
      if (info.combos[k] < 0 || info.combos[k] >= info.npm)
        return f + "combos: product " + num(j) + ": power index " + num(info.combos[k]) + " is not below npm " +
               num(info.npm);
  }
  // the columns: each (argument, column) pair inside the witness group the argument is
  if (info.ncols < 0 || info.ncols > kMaxCols) return f + "ncols: " + num(info.ncols) + " is not 0 to " + num(kMaxCols);
  if (info.ncols && (!info.col_arg || !info.col_idx)) return f + "col_arg, col_idx: NULL with ncols " + num(info.ncols);
  for (int i = 0; i < info.ncols; i++) {
    const int a = info.col_arg[i], c = info.col_idx[i];
    if (a < 0 || a >= info.nargs)
      return f + "col_arg: column " + num(i) + " names argument " + num(a) + " of " + num(info.nargs);
    const int what = t.eval_args[a];
    // a column is read at col_idx * rows + row: only a witness group is laid out that way, and a
    // mix or global argument is inside itself only as its one column 0
    const long long size = what >= 0 ? (long long)t.group_sizes[what] : 1;
    const char* name = what == 0 ? "accum" : what == 1 ? "code" : what == 2 ? "data" : what == -1 ? "mix" : "global";
    if (c < 0 || c >= size)
      return f + "col_idx: column " + num(i) + " is column " + num(c) + " of " + name + ", which has " + num(size);
  }
  if (info.n_uniform < 0 || info.n_uniform > kMaxUniform)
    return f + "n_uniform: " + num(info.n_uniform) + " is not 0 to " + num(kMaxUniform);
  if (info.n_uniform && !info.uniform) return f + "uniform: NULL with n_uniform " + num(info.n_uniform);
  // the gates: each a column of a witness group (the zero scan reads `rows` words of it)
  if (info.ngates < 0 || info.ngates > kMaxGates)
    return f + "ngates: " + num(info.ngates) + " is not 0 to " + num(kMaxGates);
  if (info.ngates && (!info.gate_col || !info.plan)) return f + "gate_col, plan: NULL with ngates " + num(info.ngates);
  for (int g = 0; g < info.ngates; g++) {
    const int i = info.gate_col[g];
    if (i < 0 || i >= info.ncols) return f + "gate_col: gate " + num(g) + " names column " + num(i) + " of " + num(info.ncols);
    if (t.eval_args[info.col_arg[i]] < 0)
      return f + "gate_col: gate " + num(g) + " is a column of mix or global, not of a witness group";
  }
  return "";
}

std::string check_module(const r0hip_module_desc* d, const Expect& want) {
  std::string bad = check_descriptor(d, want);
  if (!bad.empty()) return bad;
  bad = rt::validate(d->tables);
  if (!bad.empty()) return bad;
  const struct {
    r0hip_module_fn fn;
    const char* family;
  } views[2] = {{d->info, "info"}, {d->rows_info, "rows_info"}};
  for (const auto& v : views) {
    EvalCheckInfo info{};
    reinterpret_cast<InfoFn>(v.fn)(&info);
    bad = check_kernel_view(d->tables, info, v.family);
    if (!bad.empty()) return bad;
  }
  return "";
}

}  // namespace mod
}  // namespace r0
