// rv32im BigInt accumulator states on the GPU: BigIntAccum::step (circuit/rv32im/src/prove/
// witgen/byte_poly.rs:381-470) over all Back::BigInt records of a trace at once. bigint.cpp
// holds the serial restatement and says where the step sits in the proof; this file computes
// the same 12 words per record (poly, term, total) as three scans, each reading the exclusive
// result of the one before it:
//
//   poly   an affine scan. Record k maps poly to a_k * poly + b_k: Shift (x^16, x^16 * D_k),
//          Carry1 (1, (D_k - neg_poly) * 16384), Carry2 (1, D_k * 256), every other op (0, 0);
//          D_k = sum_i x^i * bytes[i] is the record's byte polynomial at the final mix x.
//          g after f is (g.a * f.a, g.a * f.b + g.b); the state starts at 0, so poly_k is the
//          b of the composition of records 0..k.
//   term   a last-writer scan. SetTerm writes new_poly_k = poly_{k-1} + D_k, AddTotal, Reset
//          and EqZero write 1; with no writer so far the value is 1.
//   total  a segmented sum. Reset and EqZero clear it, AddTotal adds
//          (coeff - 4) * term_{k-1} * new_poly_k.
//
// EqZero's check, total_{k-1} + new_poly_k * (x - 256) == 0, is made per record in the last
// scan; the smallest failing record index lands in one device word (atomicMin).
//
// Field arithmetic is exact and every result canonical, so the words equal the serial loop's
// whatever the order of composition. Each scan is accum.hip's three passes: per-tile sums (a
// tile is 256 lanes x 16 consecutive records), one workgroup scanning the tile sums, and the
// in-tile scan with the tile's offset; inside a workgroup wave64 shuffles, then LDS across the
// four waves. One kernel before them computes every D_k, one lane per record.
#include "../../include/r0hip.h"
#include "bb31.h"
#include "runtime.h"

namespace r0 {
namespace {

constexpr int kT = 256;   // lanes per workgroup
constexpr int kPer = 16;  // consecutive records per lane
constexpr uint32_t kTile = kT * kPer;
constexpr int kWidthBytes = 16;  // BIGINT_WIDTH_BYTES
constexpr int kRecWords = 7;     // sizeof(r0hip_bigint_back) / 4: row, poly_op, coeff, 16 bytes
static_assert(sizeof(r0hip_bigint_back) == kRecWords * 4, "r0hip_bigint_back is 28 bytes");
constexpr size_t kMixWords = 36;  // REGCOUNT_MIX
constexpr uint32_t kEnc4 = fp_encode(4), kEnc128 = fp_encode(128), kEnc256 = fp_encode(256),
                   kEnc16384 = fp_encode(64 * 256);

enum PolyOp : uint32_t { kReset = 0, kShift, kSetTerm, kAddTotal, kCarry1, kCarry2, kEqZero };  // bigint.rs:62-70

struct Args {
  const uint32_t* recs;  // n records, kRecWords words each
  uint32_t* delta;       // n x 4: D_k
  uint32_t* states;      // n x 12: poly, term, total
  uint32_t* fail;        // smallest record index with a failing EqZero
  uint32_t n;
  FpExt powers[kWidthBytes + 1];  // of the final mix
  FpExt neg_poly;                 // sum_{i<16} powers[i] * 128
  FpExt carry;                    // powers[1] - 256
};

__device__ __forceinline__ FpExt ld_fe(const uint32_t* p) { return FpExt{{p[0], p[1], p[2], p[3]}}; }
__device__ __forceinline__ void st_fe(uint32_t* p, FpExt v) {
#pragma unroll
  for (int i = 0; i < 4; i++) p[i] = v.c[i];
}
__device__ __forceinline__ uint32_t enc(uint32_t v) { return fp_mul(kR2, v % kP); }  // Elem::new
__device__ __forceinline__ uint32_t op_of(const Args& A, uint32_t k) { return A.recs[size_t(k) * kRecWords + 1]; }
__device__ __forceinline__ FpExt delta_of(const Args& A, uint32_t k) { return ld_fe(A.delta + size_t(k) * 4); }
// poly_{k-1} + D_k, the polynomial the record's op works on
__device__ __forceinline__ FpExt new_poly_of(const Args& A, uint32_t k) {
  const FpExt prev = k ? ld_fe(A.states + size_t(k - 1) * 12) : fe_zero();
  return fe_add(prev, delta_of(A, k));
}

__global__ __launch_bounds__(kT) void bigint_delta_kernel(Args A) {
  const uint32_t k = blockIdx.x * kT + threadIdx.x;
  if (k >= A.n) return;
  const uint32_t* w = A.recs + size_t(k) * kRecWords + 3;
  FpExt d = fe_zero();
#pragma unroll
  for (int i = 0; i < kWidthBytes; i++) {
    const uint32_t byte = (w[i >> 2] >> (8 * (i & 3))) & 0xFF;
    d = fe_add(d, fe_mul_fp(A.powers[i], enc(byte)));
  }
  st_fe(A.delta + size_t(k) * 4, d);
}

// ---- the three scans: element type, identity, composition (l first, then r), the element of
// record k, and what record k stores given the composition before and after it ----

struct ScanPoly {
  struct Elem {
    FpExt a, b;
  };
  static __device__ __forceinline__ Elem identity() { return Elem{fe_one(), fe_zero()}; }
  static __device__ __forceinline__ Elem combine(const Elem& l, const Elem& r) {
    return Elem{fe_mul(r.a, l.a), fe_add(fe_mul(r.a, l.b), r.b)};
  }
  static __device__ __forceinline__ Elem load(const Args& A, uint32_t k) {
    const FpExt d = delta_of(A, k);
    switch (op_of(A, k)) {
      case kShift:
        return Elem{A.powers[kWidthBytes], fe_mul(A.powers[kWidthBytes], d)};
      case kCarry1:
        return Elem{fe_one(), fe_mul_fp(fe_sub(d, A.neg_poly), kEnc16384)};
      case kCarry2:
        return Elem{fe_one(), fe_mul_fp(d, kEnc256)};
      default:  // Reset, SetTerm, AddTotal, EqZero leave poly at 0
        return Elem{fe_zero(), fe_zero()};
    }
  }
  static __device__ __forceinline__ void emit(const Args& A, uint32_t k, const Elem&, const Elem& after) {
    st_fe(A.states + size_t(k) * 12, after.b);
  }
};

struct ScanTerm {
  struct Elem {
    uint32_t has;
    FpExt v;
  };
  static __device__ __forceinline__ Elem identity() { return Elem{0u, fe_zero()}; }
  static __device__ __forceinline__ Elem combine(const Elem& l, const Elem& r) { return r.has ? r : l; }
  static __device__ __forceinline__ Elem load(const Args& A, uint32_t k) {
    switch (op_of(A, k)) {
      case kSetTerm:
        return Elem{1u, new_poly_of(A, k)};
      case kReset:
      case kAddTotal:
      case kEqZero:
        return Elem{1u, fe_one()};
      default:
        return identity();
    }
  }
  static __device__ __forceinline__ void emit(const Args& A, uint32_t k, const Elem&, const Elem& after) {
    st_fe(A.states + size_t(k) * 12 + 4, after.has ? after.v : fe_one());
  }
};

struct ScanTotal {
  struct Elem {
    uint32_t clear;
    FpExt v;
  };
  static __device__ __forceinline__ Elem identity() { return Elem{0u, fe_zero()}; }
  static __device__ __forceinline__ Elem combine(const Elem& l, const Elem& r) {
    return r.clear ? r : Elem{l.clear, fe_add(l.v, r.v)};
  }
  static __device__ __forceinline__ Elem load(const Args& A, uint32_t k) {
    switch (op_of(A, k)) {
      case kReset:
      case kEqZero:
        return Elem{1u, fe_zero()};
      case kAddTotal: {
        const uint32_t coeff = fp_sub(enc(A.recs[size_t(k) * kRecWords + 2]), kEnc4);
        const FpExt term = k ? ld_fe(A.states + size_t(k - 1) * 12 + 4) : fe_one();
        return Elem{0u, fe_mul(fe_mul_fp(term, coeff), new_poly_of(A, k))};
      }
      default:
        return identity();
    }
  }
  static __device__ __forceinline__ void emit(const Args& A, uint32_t k, const Elem& before, const Elem& after) {
    st_fe(A.states + size_t(k) * 12 + 8, after.v);
    if (op_of(A, k) == kEqZero) {  // before.v is total_{k-1}
      const FpExt goal = fe_add(before.v, fe_mul(new_poly_of(A, k), A.carry));
      if (!fe_eq(goal, fe_zero())) atomicMin(A.fail, k);
    }
  }
};

template <class E>
__device__ __forceinline__ E shfl_up_elem(const E& v, int d) {
  constexpr int kWords = sizeof(E) / 4;
  static_assert(sizeof(E) % 4 == 0, "scan elements are whole words");
  uint32_t w[kWords];
  __builtin_memcpy(w, &v, sizeof(E));
#pragma unroll
  for (int i = 0; i < kWords; i++) w[i] = __shfl_up(w[i], d, 64);
  E o;
  __builtin_memcpy(&o, w, sizeof(E));
  return o;
}

// workgroup exclusive scan of one element per lane: the composition of the lanes before this
// one. wave64 shuffles, then the wave totals through LDS (kT / 64 entries).
template <class M>
__device__ __forceinline__ typename M::Elem wg_scan_excl(const typename M::Elem& v, typename M::Elem* lds) {
  using E = typename M::Elem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  E inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const E o = shfl_up_elem(inc, d);
    if (lane >= d) inc = M::combine(o, inc);
  }
  if (lane == 63) lds[wave] = inc;
  E ex = shfl_up_elem(inc, 1);
  if (lane == 0) ex = M::identity();
  __syncthreads();
  E off = M::identity();
  for (int w = 0; w < wave; w++) off = M::combine(off, lds[w]);
  __syncthreads();
  return M::combine(off, ex);
}

// the composition of this lane's records
template <class M>
__device__ __forceinline__ typename M::Elem lane_sum(const Args& A, uint32_t base) {
  typename M::Elem agg = M::identity();
  for (int i = 0; i < kPer; i++)
    if (base + i < A.n) agg = M::combine(agg, M::load(A, base + i));
  return agg;
}

template <class M>
__global__ __launch_bounds__(kT) void bigint_tile_sums_kernel(Args A, typename M::Elem* sums) {
  __shared__ typename M::Elem lds[kT / 64];
  const typename M::Elem agg = lane_sum<M>(A, blockIdx.x * kTile + threadIdx.x * kPer);
  const typename M::Elem ex = wg_scan_excl<M>(agg, lds);
  if (threadIdx.x == kT - 1) sums[blockIdx.x] = M::combine(ex, agg);
}

// one workgroup: exclusive scan of the tile sums in place, kT at a time
template <class M>
__global__ __launch_bounds__(kT) void bigint_scan_sums_kernel(typename M::Elem* sums, uint32_t ntiles) {
  using E = typename M::Elem;
  __shared__ E lds[kT / 64];
  __shared__ E chunk;
  E carry = M::identity();
  for (uint32_t b = 0; b < ntiles; b += kT) {
    const uint32_t i = b + threadIdx.x;
    const E v = i < ntiles ? sums[i] : M::identity();
    const E ex = wg_scan_excl<M>(v, lds);
    if (i < ntiles) sums[i] = M::combine(carry, ex);
    if (threadIdx.x == kT - 1) chunk = M::combine(ex, v);
    __syncthreads();
    carry = M::combine(carry, chunk);
    __syncthreads();
  }
}

template <class M>
__global__ __launch_bounds__(kT) void bigint_tile_scan_kernel(Args A, const typename M::Elem* sums) {
  using E = typename M::Elem;
  __shared__ E lds[kT / 64];
  const uint32_t base = blockIdx.x * kTile + threadIdx.x * kPer;
  const E ex = wg_scan_excl<M>(lane_sum<M>(A, base), lds);
  E acc = M::combine(sums[blockIdx.x], ex);
  for (int i = 0; i < kPer; i++) {
    const uint32_t k = base + i;
    if (k >= A.n) break;
    const E next = M::combine(acc, M::load(A, k));
    M::emit(A, k, acc, next);
    acc = next;
  }
}

template <class M>
void scan(hipStream_t s, const Args& A, void* sums, uint32_t ntiles) {
  auto* e = static_cast<typename M::Elem*>(sums);
  hipLaunchKernelGGL(bigint_tile_sums_kernel<M>, dim3(ntiles), dim3(kT), 0, s, A, e);
  hipLaunchKernelGGL(bigint_scan_sums_kernel<M>, dim3(1), dim3(kT), 0, s, e, ntiles);
  hipLaunchKernelGGL(bigint_tile_scan_kernel<M>, dim3(ntiles), dim3(kT), 0, s, A, e);
}

}  // namespace

void bigint_accum_scan(hipStream_t s, uint32_t* d_states, const r0hip_bigint_back* d_backs, size_t n,
                       const uint32_t* mix, uint32_t* d_fail) {
  HIP_OK(hipMemsetD32Async(d_fail, 0xFFFFFFFFu, 1, s));
  if (n == 0) return;
  R0_REQUIRE(n <= (size_t(1) << 26), "bigint_accum_scan: more than 2^26 records");
  KScope ks("bigint_accum", double(n) * (28 + 3 * 16 + 5 * 48), double(n) * 120);
  Args A{};
  A.recs = reinterpret_cast<const uint32_t*>(d_backs);
  A.delta = static_cast<uint32_t*>(scratch(n * 16, kSlotBigIntDelta));
  A.states = d_states;
  A.fail = d_fail;
  A.n = uint32_t(n);
  // BigIntAccum::new (byte_poly.rs:381-401) with the final mix (witgen/mod.rs:184)
  const FpExt x{{mix[kMixWords - 4], mix[kMixWords - 3], mix[kMixWords - 2], mix[kMixWords - 1]}};
  FpExt cur = fe_one();
  for (auto& p : A.powers) {
    p = cur;
    cur = fe_mul(cur, x);
  }
  A.neg_poly = fe_zero();
  for (int i = 0; i < kWidthBytes; i++) A.neg_poly = fe_add(A.neg_poly, fe_mul_fp(A.powers[i], kEnc128));
  A.carry = fe_sub(A.powers[1], fe_from_fp(kEnc256));
  const uint32_t ntiles = uint32_t((n + kTile - 1) / kTile);
  void* sums = scratch(size_t(ntiles) * sizeof(ScanPoly::Elem), kSlotBigIntTileSums);
  hipLaunchKernelGGL(bigint_delta_kernel, dim3(div_up(n, kT)), dim3(kT), 0, s, A);
  scan<ScanPoly>(s, A, sums, ntiles);
  scan<ScanTerm>(s, A, sums, ntiles);
  scan<ScanTotal>(s, A, sums, ntiles);
  HIP_OK(hipGetLastError());
}

}  // namespace r0
