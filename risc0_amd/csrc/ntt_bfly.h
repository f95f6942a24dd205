// Range-typed BabyBear helpers and the butterfly network of one NTT register group
// (ntt.hip stage_group), shared by the kernels and the host test
// (tests/native/ntt_bfly_equiv.cpp).
//
// mont_reduce is correct for any t < p * 2^32, so the operand of a Montgomery product
// that meets a canonical twiddle may be any 32-bit word. A sum of two canonical words is
// below 2p < 2^32 and a difference plus p lies in [1, 2p): neither needs its sub/min pair
// when its only consumer is such a product. Three ranges of a word appear below:
//   canonical  < p       everything in memory and LDS, every addend, every twiddle
//   lazy       < 2p      fp_add_lazy, fp_sub_lazy, fp_mul_wide_lazy results
//   wide       < 2^32    what fp_mul_wide* accept as their first operand
// A lazy word is never added to or subtracted from: p = 15 * 2^27 + 1 leaves one bit of
// headroom in 32 bits, so a second addition could wrap.
#pragma once
#include "bb31.h"

// R0_NTT_BFLY_CHECK (host test only): every range stated below is asserted where it is used
#if defined(R0_NTT_BFLY_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
#include <assert.h>
#define R0_BFLY_RANGE(c) assert(c)
#else
#define R0_BFLY_RANGE(c) ((void)0)
#endif

namespace r0 {

static_assert(2 * uint64_t(kP) <= (uint64_t(1) << 32), "a lazy word (< 2p) must fit 32 bits");
// fp_mul_wide: t = y * w <= (2^32 - 1)(p - 1) < p * 2^32 (mont_reduce's bound), and
// t + m * p < 2 * p * 2^32 does not wrap 64 bits
static_assert(kP < (uint64_t(1) << 31), "t + m*p < p * 2^33 must fit 64 bits");

// a, b < p -> a + b mod p as a word < 2p (one add)
R0_HD uint32_t fp_add_lazy(uint32_t a, uint32_t b) {
  R0_BFLY_RANGE(a < kP && b < kP);
  return a + b;
}
// a, b < p -> a - b mod p as a word in [1, 2p) (sub, add)
R0_HD uint32_t fp_sub_lazy(uint32_t a, uint32_t b) {
  R0_BFLY_RANGE(a < kP && b < kP);
  return a - b + kP;
}
// any y < 2^32, w < p -> y * w * 2^-32 mod p, before the last fold: < 2p. Only for a
// result that is the first operand of another fp_mul_wide*.
R0_HD uint32_t fp_mul_wide_lazy(uint32_t y, uint32_t w) {
  R0_BFLY_RANGE(w < kP);
  const uint64_t t = uint64_t(y) * w;  // < p * 2^32
  const uint32_t m = uint32_t(t) * kNegPinv;
  return uint32_t((t + uint64_t(m) * kP) >> 32);  // < (p * 2^32 + 2^32 * p) / 2^32 = 2p
}
// any y < 2^32, w < p -> y * w * 2^-32 mod p, canonical
R0_HD uint32_t fp_mul_wide(uint32_t y, uint32_t w) {
  const uint32_t r = fp_mul_wide_lazy(y, w);
  return umin(r, r - kP);
}

// ---- one register group of NST radix-2 stages ------------------------------------
// v[m], m < 2^NST, are the group's elements in stage order (element m of stage st pairs
// with m + 2^st); tw(st, q) is the canonical twiddle of stage st for the pair whose low
// index bits are q = m & (2^st - 1). TRIV: the group starts at the transform's first
// stage, where tw(st, 0) = 1 and that multiply is skipped.
//
// Forward (DIT): (x, y) -> (x + y*w, x - y*w). The output at index i of stage st is left
// lazy exactly when its next use inside the group is the multiplied operand of a
// multiply that is not skipped; addends (the x side), operands of a skipped multiply and
// the words that leave the group stay canonical.
constexpr bool bfly_fwd_lazy(int NST, bool TRIV, int st, uint32_t i) {
  const uint32_t nh = 2u << st;  // the next stage's half
  return st + 1 < NST && (i & nh) != 0 && !(TRIV && (i & (nh - 1)) == 0);
}
// lazy outputs of a whole forward group (for the counts quoted in DESIGN.md)
constexpr int bfly_fwd_lazy_count(int NST, bool TRIV) {
  int n = 0;
  for (int st = 0; st < NST; st++)
    for (uint32_t i = 0; i < (1u << NST); i++) n += bfly_fwd_lazy(NST, TRIV, st, i) ? 1 : 0;
  return n;
}
static_assert(bfly_fwd_lazy_count(3, false) == 8, "half of the outputs of stages 0 and 1");
static_assert(bfly_fwd_lazy_count(3, true) == 5, "less the operands of the skipped multiplies");
static_assert(bfly_fwd_lazy_count(1, false) == 0, "everything that leaves the group is canonical");
static_assert(bfly_fwd_lazy(3, false, 0, 2) && bfly_fwd_lazy(3, false, 0, 3) && bfly_fwd_lazy(3, false, 1, 4) &&
                  !bfly_fwd_lazy(3, false, 0, 4) && !bfly_fwd_lazy(3, false, 2, 7),
              "m in {2,3,6,7} after stage 0, {4,5,6,7} after stage 1, none after the last");

// Inverse (DIF): (x, y) -> (x + y, (x - y)*w), stages descending. Both inputs are addends,
// so only the difference, which goes straight into its multiply, is lazy.
template <int NST, bool INV, bool TRIV, typename TW>
R0_HD void bfly_group(uint32_t (&v)[1 << NST], const TW& tw) {
  constexpr uint32_t M = 1u << NST;
  if (!INV) {
#pragma unroll
    for (int st = 0; st < NST; st++) {
      const uint32_t half = 1u << st;
#pragma unroll
      for (uint32_t m = 0; m < M; m++) {
        if (m & half) continue;
        const uint32_t q = m & (half - 1);
        const uint32_t x = v[m];
        uint32_t y = v[m + half];
        if (!(TRIV && q == 0)) y = fp_mul_wide(y, tw(uint32_t(st), q));
        R0_BFLY_RANGE(x < kP && y < kP);
        v[m] = bfly_fwd_lazy(NST, TRIV, st, m) ? fp_add_lazy(x, y) : fp_add(x, y);
        v[m + half] = bfly_fwd_lazy(NST, TRIV, st, m + half) ? fp_sub_lazy(x, y) : fp_sub(x, y);
      }
    }
  } else {
#pragma unroll
    for (int st = NST - 1; st >= 0; st--) {
      const uint32_t half = 1u << st;
#pragma unroll
      for (uint32_t m = 0; m < M; m++) {
        if (m & half) continue;
        const uint32_t q = m & (half - 1);
        const uint32_t x = v[m], y = v[m + half];
        R0_BFLY_RANGE(x < kP && y < kP);
        v[m] = fp_add(x, y);
        if (TRIV && q == 0) v[m + half] = fp_sub(x, y);
        else v[m + half] = fp_mul_wide(fp_sub_lazy(x, y), tw(uint32_t(st), q));
      }
    }
  }
#pragma unroll
  for (uint32_t m = 0; m < M; m++) R0_BFLY_RANGE(v[m] < kP);
}

}  // namespace r0
