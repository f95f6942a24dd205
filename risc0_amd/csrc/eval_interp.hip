// The constraint program of a circuit registered at run time, interpreted on the device
// (circuit_rt.h has the bytecode; prover.cpp run_eval_check / constraint_rows_run branch here when
// CircuitDef::interp is set). Two entry points share one evaluation loop:
//   eval_check form       over the 4 * 2^po2 domain, a tap 4 * back points behind, the result times
//                         vinv[i & 3] into the four planes of `check`, as the generated family's
//                         last kernel writes it
//   constraint_rows form  over the 2^po2 rows, a tap back rows behind, no scale, one FpExt per row
//                         (AoS) into `acc`
// One lane per point. The record index and the record array are the same in every lane, so a
// wave reads each record at one address (scalar loads) and the opcode and operand-kind switches
// are uniform branches: no lane of a wave ever takes another path than its neighbours. A lane's
// values live in a slot file in device memory, slot-major (slot * lanes + lane; an FpExt slot is
// four such planes), so a wave's access to one slot is one contiguous line. There is no per-lane
// array: a local array indexed by a run-time slot number would live in scratch memory.
// The points are taken in chunks, one launch each, sized so that the slot file stays under
// kInterpSlotBudget; the last chunk may be short, and lanes past a chunk's end return before
// their first load. Everything a record can address was checked on the host when the circuit was
// registered (circuit_rt.cpp validate): slots are below the counts the file is sized by, tap,
// word, constant and power indices below their tables' lengths.
#include <algorithm>

#include "circuit_rt.h"
#include "eval_interp.h"
#include "runtime.h"

namespace r0 {

namespace {

constexpr int kThreads = 256;

// What every lane reads at the same address and no kernel writes. The kernels take these as
// __restrict__ parameters of their own: only then does the compiler know that the slot-file
// stores cannot change them, and reads them with scalar loads.
struct InterpTables {
  const uint32_t* const* args;  // device table: the eval_check argument buffers
  const rt::Record* code;
  const uint32_t* consts;
  const rt::TapRef* taps;
  const uint32_t* pow;  // the poly_mix powers, FpExt AoS
};

struct InterpArgs {
  uint32_t* fp_slots;   // [slot][lanes]
  uint32_t* ext_slots;  // [slot][4][lanes]
  const uint32_t* vinv;
  uint32_t* check;  // eval_check form: 4 x n
  uint32_t* acc;    // rows form: n x FpExt
  uint32_t n_code;
  uint32_t lanes;  // the slot file's lane count (the chunk size)
  uint32_t n;      // domain or rows, a power of two
  uint32_t base, count;  // this launch's points: [base, base + count)
};

__device__ __forceinline__ FpExt load_ext4(const uint32_t* p) { return FpExt{{p[0], p[1], p[2], p[3]}}; }

// One operand as an FpExt (an Fp value in component 0). `kind` and `v` are wave-uniform.
__device__ __forceinline__ FpExt load_operand(const InterpArgs& A, const InterpTables& T, uint32_t kind, uint32_t v,
                                              uint32_t lane, uint32_t i) {
  switch (kind) {
    case rt::K_FP_SLOT:
      return fe_from_fp(A.fp_slots[size_t(v) * A.lanes + lane]);
    case rt::K_EXT_SLOT: {
      const uint32_t* p = A.ext_slots + size_t(v) * 4 * A.lanes + lane;
      return FpExt{{p[0], p[A.lanes], p[size_t(2) * A.lanes], p[size_t(3) * A.lanes]}};
    }
    case rt::K_FP_IMM:
      return fe_from_fp(v);
    case rt::K_EXT_IMM:
      return load_ext4(T.consts + size_t(v) * 4);
    case rt::K_WORD:
      return fe_from_fp(T.args[v >> 24][v & 0xFFFFFFu]);
    case rt::K_TAP: {
      const rt::TapRef t = T.taps[v];
      return fe_from_fp(T.args[t.arg][size_t(t.col) * A.n + ((i - t.back) & (A.n - 1))]);
    }
    default:
      return fe_zero();
  }
}

template <bool ROWS>
__global__ __launch_bounds__(kThreads) void interp_kernel(InterpArgs A, const uint32_t* const* __restrict__ args,
                                                          const rt::Record* __restrict__ code,
                                                          const uint32_t* __restrict__ consts,
                                                          const rt::TapRef* __restrict__ taps,
                                                          const uint32_t* __restrict__ pow) {
  const InterpTables T{args, code, consts, taps, pow};
  const uint32_t lane = blockIdx.x * kThreads + threadIdx.x;
  if (lane >= A.count) return;  // past the chunk's end: no load, no store
  const uint32_t i = A.base + lane;
  for (uint32_t pc = 0; pc < A.n_code; pc++) {
    const rt::Record r = T.code[pc];
    const uint32_t base = r.op >> 2;
    const bool xe = r.op & 1, ye = r.op & 2;
    const FpExt x = load_operand(A, T, r.kinds & 15, r.x, lane, i);
    if (base == rt::B_RET) {
      if (ROWS) {
        reinterpret_cast<uint4*>(A.acc)[i] = make_uint4(x.c[0], x.c[1], x.c[2], x.c[3]);
      } else {
        const FpExt s = fe_mul_fp(x, A.vinv[i & 3]);
#pragma unroll
        for (int k = 0; k < 4; k++) A.check[size_t(k) * A.n + i] = s.c[k];
      }
      return;
    }
    FpExt res;
    bool res_ext = xe || ye;
    switch (base) {
      case rt::B_ADD:
        res = fe_add(x, load_operand(A, T, (r.kinds >> 4) & 15, r.y, lane, i));
        break;
      case rt::B_SUB:
        res = fe_sub(x, load_operand(A, T, (r.kinds >> 4) & 15, r.y, lane, i));
        break;
      case rt::B_MUL: {
        const FpExt y = load_operand(A, T, (r.kinds >> 4) & 15, r.y, lane, i);
        if (xe && ye) res = fe_mul(x, y);
        else if (xe) res = fe_mul_fp(x, y.c[0]);
        else if (ye) res = fe_mul_fp(y, x.c[0]);
        else res = fe_from_fp(fp_mul(x.c[0], y.c[0]));
        break;
      }
      case rt::B_ACC_A: {
        const FpExt acc = load_operand(A, T, (r.kinds >> 8) & 15, r.acc, lane, i);
        const FpExt pw = load_ext4(T.pow + size_t(r.k) * 4);
        res = fe_add(acc, xe ? fe_mul(x, pw) : fe_mul_fp(pw, x.c[0]));
        res_ext = true;
        break;
      }
      default: {  // B_ACC_B
        const FpExt y = load_operand(A, T, (r.kinds >> 4) & 15, r.y, lane, i);
        const FpExt acc = load_operand(A, T, (r.kinds >> 8) & 15, r.acc, lane, i);
        const FpExt pw = load_ext4(T.pow + size_t(r.k) * 4);
        FpExt t;
        if (xe && ye) t = fe_mul(fe_mul(x, y), pw);
        else if (xe) t = fe_mul(fe_mul_fp(x, y.c[0]), pw);
        else if (ye) t = fe_mul(fe_mul_fp(y, x.c[0]), pw);
        else t = fe_mul_fp(pw, fp_mul(x.c[0], y.c[0]));
        res = fe_add(acc, t);
        res_ext = true;
        break;
      }
    }
    if (res_ext) {
      uint32_t* p = A.ext_slots + size_t(r.dst) * 4 * A.lanes + lane;
      p[0] = res.c[0];
      p[A.lanes] = res.c[1];
      p[size_t(2) * A.lanes] = res.c[2];
      p[size_t(3) * A.lanes] = res.c[3];
    } else {
      A.fp_slots[size_t(r.dst) * A.lanes + lane] = res.c[0];
    }
  }
}

thread_local uint32_t t_test_chunk = 0;

}  // namespace

uint32_t set_interp_test_chunk(uint32_t points) noexcept {
  const uint32_t was = t_test_chunk;
  t_test_chunk = points;
  return was;
}

std::vector<uint32_t> interp_device_image(const rt::Programs& p) {
  std::vector<uint32_t> img;
  auto put = [&](const void* src, size_t bytes) {
    const uint32_t* w = static_cast<const uint32_t*>(src);
    img.insert(img.end(), w, w + bytes / 4);
  };
  put(p.code.data(), p.code.size() * sizeof(rt::Record));
  put(p.taps_check.data(), p.taps_check.size() * sizeof(rt::TapRef));
  put(p.taps_rows.data(), p.taps_rows.size() * sizeof(rt::TapRef));
  put(p.consts.data(), p.consts.size() * 4);
  if (img.empty()) img.push_back(0);
  return img;
}

uint32_t interp_chunk_points(const rt::Programs& p, size_t n) {
  size_t chunk = t_test_chunk;
  if (!chunk) {
    const size_t per_point = 4 * std::max<size_t>(1, p.slot_words());
    chunk = std::max<size_t>(kThreads, kInterpSlotBudget / per_point / kThreads * kThreads);
  }
  return uint32_t(std::min(chunk, n));
}

void eval_interp(hipStream_t s, bool rows, const rt::Programs& p, const uint32_t* d_image,
                 const uint32_t* const* d_args, const uint32_t* d_pow, size_t n, uint32_t* d_slots, uint32_t lanes,
                 const uint32_t* d_vinv, uint32_t* d_check, uint32_t* d_acc) {
  R0_REQUIRE(n > 0 && (n & (n - 1)) == 0 && n <= (size_t(1) << 26), "eval_interp: the point count is not a power of two");
  R0_REQUIRE(lanes > 0 && lanes <= n, "eval_interp: bad chunk");
  R0_REQUIRE(!p.code.empty(), "eval_interp: empty program");
  InterpArgs A{};
  InterpTables T{};
  T.args = d_args;
  T.code = reinterpret_cast<const rt::Record*>(d_image);
  const uint32_t* after = d_image + p.code.size() * (sizeof(rt::Record) / 4);
  const size_t tap_words = p.taps_check.size() * (sizeof(rt::TapRef) / 4);
  T.taps = reinterpret_cast<const rt::TapRef*>(rows ? after + tap_words : after);
  T.consts = after + 2 * tap_words;
  T.pow = d_pow;
  A.fp_slots = d_slots;
  A.ext_slots = d_slots + size_t(p.n_fp_slots) * lanes;
  A.vinv = d_vinv;
  A.check = d_check;
  A.acc = d_acc;
  A.n_code = uint32_t(p.code.size());
  A.lanes = lanes;
  A.n = uint32_t(n);
  for (size_t base = 0; base < n; base += lanes) {
    A.base = uint32_t(base);
    A.count = uint32_t(std::min<size_t>(lanes, n - base));
    if (rows)
      hipLaunchKernelGGL(interp_kernel<true>, dim3(div_up(A.count, kThreads)), dim3(kThreads), 0, s, A, T.args, T.code, T.consts,
                         T.taps, T.pow);
    else
      hipLaunchKernelGGL(interp_kernel<false>, dim3(div_up(A.count, kThreads)), dim3(kThreads), 0, s, A, T.args, T.code, T.consts,
                         T.taps, T.pow);
    HIP_OK(hipGetLastError());
  }
}

}  // namespace r0
