// The two plain structs that travel between the host driver and a circuit's generated kernels
// (evalcheck.h). No HIP header: a circuit module's descriptor (include/r0hip_module.h) states
// their sizes, and the load path's host checks (circuit_module.cpp) read EvalCheckInfo in
// programs that link no HIP. A change to either struct changes R0HIP_MODULE_ABI, with the one
// exception recorded in include/r0hip_module.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace r0 {

// the most gates a generated program may name (EvalCheckInfo::ngates): the bits of EvalCheckArgs::dead
constexpr int kMaxGates = 64;

struct EvalCheckArgs {
  const uint32_t* const* args;  // poly_fp argument buffers, circuit order
  size_t nargs;
  const uint32_t* const* colptr;  // device table: base pointer of every column the program reads
  const uint32_t* poly_mix;     // poly_mix powers + folded products (FpExt AoS, Montgomery)
  const uint32_t* poly_mix_nb;  // the same table times NBETA = -11 (lazy extension products)
  uint32_t* acc;                // scratch: domain x FpExt
  uint32_t* check;              // out: 4 x domain
  const uint32_t* vinv;         // 4 values: inv((3 w^c)^N - 1) for c = 0..3
  uint32_t* mat_fp;             // scratch: mat_fp x domain words
  uint32_t* mat_ext;            // scratch: mat_ext x domain FpExt
  uint32_t domain;
  uint32_t tile = 0;            // points per tile (0 = whole domain per launch)
  int64_t wide = -1;            // bit k: kernel k addresses taps from colptr (-1 = tuned default)
  const uint32_t* uniform = nullptr;  // info.uniform's table (4 words per value), on the device
  // bit g: the column of gate g (info.gate_col) is zero in all `domain` points, so the kernels that
  // info.plan leaves out for this mask are not launched (0 = every kernel, whatever the columns hold)
  uint64_t dead = 0;
};

struct EvalCheckInfo {
  const int* combos;  // for each folded product: count, then indices into the powers
  int ncombos;
  int npm;            // number of poly_mix powers the kernels index directly
  int nargs;
  int mat_fp, mat_ext, kernels;
  double modmuls_per_point;  // field multiplications of the restated poly_fp (+4 for the 1/Z scale)
  int ncols;             // columns the program reads: (argument, column) pairs
  const int* col_arg;
  const int* col_idx;
  // lane-independent values the kernels read (4 words each), evaluated on the host from host
  // copies of the eval_check arguments (only mix and global are read: g[i] null otherwise)
  // and the poly_mix powers (FpExt AoS)
  int n_uniform;
  void (*uniform)(const uint32_t* const* g, const uint32_t* poly_mix, uint32_t* out);
  // gates: columns that enter terms of poly_fp as a plain factor, as indices into col_arg/col_idx
  // (at most kMaxGates). A gate whose column is zero everywhere makes its terms contribute 0; plan(dead)
  // is the set of kernels (bit k, of `kernels`) the launcher runs for the mask `dead` of such gates.
  int ngates;
  const int* gate_col;
  uint64_t (*plan)(uint64_t dead);
};

}  // namespace r0
