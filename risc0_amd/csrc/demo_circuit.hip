// The demo circuit's device side (risc0_amd/circuits/demo.*, tools/gen_demo_circuit.py): a
// valid witness and its accumulation, so the library can prove a circuit end to end on its own
// (r0hip_selftest) and the plug-in path has an example in the tree.
//
//   witness : row i of the active rows holds (a_i, b_i) = M^i (a_0, b_0), M = [[0, 1], [1, 1]],
//             and s_i = a_i * b_i. One lane per row raises M to its row by squaring (M's powers
//             are [[x, y], [y, x + y]], two words), so no lane waits for another row.
//   accum   : z_i = sum over j <= i of m * a_j, m the FpExt of the four mix words: a sum scan in
//             three passes (sums of 1024-row tiles, one workgroup scanning the tile sums, the scan
//             inside each tile on top of its tile's prefix).
// Both are a few words per row and far from any limit of the card; they have to be right at every
// size the prover takes, not fast. Every word written is canonical.
#include "bb31.h"
#include "devmem.h"
#include "plugin.h"
#include "runtime.h"

namespace r0 {
namespace {

constexpr int kT = 256;
constexpr int kPer = 4;
constexpr uint32_t kTile = kT * kPer;

// powers of M as (x, y) for [[x, y], [y, x + y]]
struct Sym {
  uint32_t x, y;
};
__device__ __forceinline__ Sym sym_mul(Sym p, Sym q) {
  const uint32_t yy = fp_mul(p.y, q.y);
  return Sym{fp_add(fp_mul(p.x, q.x), yy), fp_add(fp_add(fp_mul(p.x, q.y), fp_mul(p.y, q.x)), yy)};
}

__global__ __launch_bounds__(kT) void demo_witness_kernel(uint32_t rows, uint32_t n, uint32_t a0, uint32_t b0,
                                                          uint32_t* code, uint32_t* data, uint32_t* global) {
  const uint32_t i = blockIdx.x * kT + threadIdx.x;
  if (i >= rows) return;
  code[i] = i == 0 ? kOne : 0u;                      // first
  code[size_t(rows) + i] = i < n ? kOne : 0u;        // on
  code[2 * size_t(rows) + i] = i == n - 1 ? kOne : 0u;  // last
  if (i >= n) return;
  Sym r{kOne, 0u}, p{0u, kOne};
  for (uint32_t e = i; e; e >>= 1) {
    if (e & 1) r = sym_mul(r, p);
    p = sym_mul(p, p);
  }
  const uint32_t a = fp_add(fp_mul(r.x, a0), fp_mul(r.y, b0));
  const uint32_t b = fp_add(fp_mul(r.y, a0), fp_mul(fp_add(r.x, r.y), b0));
  data[i] = a;
  data[size_t(rows) + i] = b;
  data[2 * size_t(rows) + i] = fp_mul(a, b);
  if (i == 0) {
    global[0] = a;
    global[1] = b;
  }
  if (i == n - 1) global[2] = b;
}

__device__ __forceinline__ FpExt ld4(const uint4* p) {
  const uint4 v = *p;
  return FpExt{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void st4(uint4* p, const FpExt& a) { *p = make_uint4(a.c[0], a.c[1], a.c[2], a.c[3]); }
__device__ __forceinline__ FpExt shfl_up4(const FpExt& a, int d) {
  FpExt r;
#pragma unroll
  for (int i = 0; i < 4; i++) r.c[i] = __shfl_up(a.c[i], d, 64);
  return r;
}

// workgroup inclusive sum scan of one FpExt per lane; lds keeps the per-wave totals
__device__ FpExt wg_scan_add(FpExt v, FpExt* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const FpExt o = shfl_up4(v, d);
    if (lane >= d) v = fe_add(v, o);
  }
  __syncthreads();  // the totals of an earlier scan have been read
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  FpExt off = fe_zero();
  for (int w = 0; w < wave; w++) off = fe_add(off, lds[w]);
  return fe_add(v, off);
}

struct Mix {
  uint32_t w[4];
};

// this lane's kPer terms m * a_row (zero above n) and their sum
__device__ __forceinline__ FpExt lane_terms(const uint32_t* a, uint32_t n, const Mix& m, FpExt (&x)[kPer]) {
  const uint64_t base = uint64_t(blockIdx.x) * kTile + uint64_t(threadIdx.x) * kPer;
  const FpExt mm{{m.w[0], m.w[1], m.w[2], m.w[3]}};
  FpExt sum = fe_zero();
#pragma unroll
  for (int i = 0; i < kPer; i++) {
    x[i] = base + i < n ? fe_mul_fp(mm, a[base + i]) : fe_zero();
    sum = fe_add(sum, x[i]);
  }
  return sum;
}

__global__ __launch_bounds__(kT) void demo_tile_sums_kernel(const uint32_t* a, uint32_t n, Mix m, uint4* sums) {
  __shared__ FpExt lds[kT / 64];
  FpExt x[kPer];
  const FpExt inc = wg_scan_add(lane_terms(a, n, m, x), lds);
  if (threadIdx.x == kT - 1) st4(sums + blockIdx.x, inc);
}

// one workgroup: exclusive sum scan of the tile sums, in place
__global__ __launch_bounds__(kT) void demo_scan_sums_kernel(uint4* sums, uint32_t ntiles) {
  __shared__ FpExt lds[kT / 64];
  __shared__ FpExt total;
  FpExt carry = fe_zero();
  for (uint32_t b = 0; b < ntiles; b += kT) {
    const uint32_t i = b + threadIdx.x;
    const FpExt v = i < ntiles ? ld4(sums + i) : fe_zero();
    const FpExt inc = wg_scan_add(v, lds);
    if (i < ntiles) st4(sums + i, fe_add(carry, fe_sub(inc, v)));
    if (threadIdx.x == kT - 1) total = inc;
    __syncthreads();
    carry = fe_add(carry, total);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kT) void demo_apply_kernel(const uint32_t* a, uint32_t rows, uint32_t n, Mix m,
                                                        const uint4* sums, uint32_t* accum) {
  __shared__ FpExt lds[kT / 64];
  FpExt x[kPer];
  const FpExt sum = lane_terms(a, n, m, x);
  const FpExt inc = wg_scan_add(sum, lds);
  FpExt run = fe_add(ld4(sums + blockIdx.x), fe_sub(inc, sum));
  const uint64_t base = uint64_t(blockIdx.x) * kTile + uint64_t(threadIdx.x) * kPer;
#pragma unroll
  for (int i = 0; i < kPer; i++) {
    run = fe_add(run, x[i]);
    if (base + i < n) {
#pragma unroll
      for (int k = 0; k < 4; k++) accum[size_t(k) * rows + base + i] = run.c[k];
    }
  }
}

void check_shape(const char* who, uint32_t po2, size_t n) {
  R0_REQUIRE(po2 >= 2 && po2 <= 24, std::string(who) + ": po2 " + std::to_string(po2) + " out of range (2..24)");
  R0_REQUIRE(n >= 1 && n <= (size_t(1) << po2),
             std::string(who) + ": n_active " + std::to_string(n) + " is not in 1..2^po2");
}

}  // namespace

void demo_witness(hipStream_t s, uint32_t po2, size_t n, uint32_t a0, uint32_t b0, uint32_t* code, uint32_t* data,
                  uint32_t* global) {
  check_shape("demo_witness", po2, n);
  R0_REQUIRE(a0 < kP && b0 < kP, "demo_witness: a0, b0 must be canonical words");
  R0_REQUIRE(code && data && global, "demo_witness: null argument");
  const uint32_t rows = uint32_t(1) << po2;
  KScope ks("demo_witness", double(rows) * 6 * 4);
  hipLaunchKernelGGL(demo_witness_kernel, dim3(div_up(rows, kT)), dim3(kT), 0, s, rows, uint32_t(n), a0, b0, code, data,
                     global);
  HIP_OK(hipGetLastError());
}

void demo_accum(hipStream_t s, uint32_t po2, size_t n, const uint32_t* data, const uint32_t* h_mix, uint32_t* accum) {
  check_shape("demo_accum", po2, n);
  R0_REQUIRE(data && h_mix && accum, "demo_accum: null argument");
  Mix m;
  for (int k = 0; k < 4; k++) {
    R0_REQUIRE(h_mix[k] < kP, "demo_accum: a mix word is not canonical");
    m.w[k] = h_mix[k];
  }
  const uint32_t rows = uint32_t(1) << po2;
  const uint32_t ntiles = uint32_t((n + kTile - 1) / kTile);
  KScope ks("demo_accum", double(n) * 6 * 4);
  DevBuf sums(size_t(ntiles) * 4);  // freed to this thread's pool: reused in stream order only
  uint4* ts = reinterpret_cast<uint4*>(sums.p);
  hipLaunchKernelGGL(demo_tile_sums_kernel, dim3(ntiles), dim3(kT), 0, s, data, uint32_t(n), m, ts);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(demo_scan_sums_kernel, dim3(1), dim3(kT), 0, s, ts, ntiles);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(demo_apply_kernel, dim3(ntiles), dim3(kT), 0, s, data, rows, uint32_t(n), m, ts, accum);
  HIP_OK(hipGetLastError());
}

}  // namespace r0
