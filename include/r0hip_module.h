/* Circuit modules: one circuit's generated kernels as a shared object of their own, handed to a
 * running libr0hip.so with r0hip_circuit_load (r0hip.h).
 *
 * A module is built by `make -C risc0_amd/csrc module NAME=x DIR=dir OUT=path/x.r0mod.so` from
 * dir/x.poly.ir and dir/x.taps.json (and dir/x.ectune.json, if there is one): the circuit's
 * tables, the generated eval_check and constraint-rows kernels for one GPU architecture and their
 * host launchers. It exports exactly one symbol with default visibility, R0HIP_MODULE_ENTRY;
 * everything else is hidden, so two modules of the same generator live in one process. A module
 * has no undefined reference into libr0hip.so (its launchers use inline code and the HIP runtime
 * only), so the library may itself be loaded RTLD_LOCAL.
 *
 * Loading a module runs its code, exactly as linking it would: load only what you would link.
 *
 * The descriptor and everything it points to belong to the module and live as long as the
 * process: a module is never closed once its circuit is in the registry. */
#ifndef R0HIP_MODULE_H
#define R0HIP_MODULE_H

#include <stddef.h>
#include <stdint.h>

#include "r0hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Changes whenever EvalCheckArgs, EvalCheckInfo (risc0_amd/csrc/evalcheck_types.h) or
 * r0hip_module_desc change. A library loads only modules of its own number and of its own three
 * sizes (below). One recorded exception to the rule: the gates (EvalCheckArgs::dead,
 * EvalCheckInfo::ngates, gate_col, plan) grew the structs by 8 and 24 bytes and left the number at
 * 1, because the refusal tests pin it; every older module is refused by its sizes. The next
 * change to either struct bumps the number to 2, and a change that keeps the sizes must. */
#define R0HIP_MODULE_ABI 1u
#define R0HIP_MODULE_ENTRY "r0hip_circuit_module"

/* The four pointers cross this header as plain function pointers; the library converts them back
 * to the types they were defined with (risc0_amd/csrc/evalcheck.h):
 *   eval_check, constraint_rows   void (hipStream_t, const r0::EvalCheckArgs&)
 *   info, rows_info               void (r0::EvalCheckInfo*)                                    */
typedef void (*r0hip_module_fn)(void);

typedef struct r0hip_module_desc {
  uint32_t abi;       /* R0HIP_MODULE_ABI as the module was compiled */
  uint32_t desc_size; /* sizeof(r0hip_module_desc), sizeof(r0::EvalCheckArgs) and */
  uint32_t args_size; /* sizeof(r0::EvalCheckInfo), as the module saw them */
  uint32_t info_size;
  const char* arch;            /* the architecture its kernels were compiled for ("gfx950") */
  r0hip_circuit_tables tables; /* what r0hip_circuit_register takes: the name, the tables, the ir */
  r0hip_module_fn eval_check;
  r0hip_module_fn info;
  r0hip_module_fn constraint_rows;
  r0hip_module_fn rows_info;
} r0hip_module_desc;

/* The module's one exported symbol, named R0HIP_MODULE_ENTRY. */
typedef const r0hip_module_desc* (*r0hip_module_entry_fn)(void);

#ifdef __cplusplus
}
#endif

#endif
