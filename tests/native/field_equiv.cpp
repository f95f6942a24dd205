// Host-side equivalence checks of the product's lean field/hash formulations against
// their step-by-step restatements (tests/test_host_arith.py builds and runs this).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "poseidon2.h"

using namespace r0;

static int fails = 0;
#define EXPECT(c, ...)            \
  do {                            \
    if (!(c)) {                   \
      if (fails++ < 10) std::printf(__VA_ARGS__); \
    }                             \
  } while (0)

// reference extension multiply: baby_bear.rs:744-757 with canonical ops only
static FpExt fe_mul_simple(FpExt a, FpExt b) {
  uint32_t r[4];
  for (int k = 0; k < 4; k++) r[k] = 0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      uint32_t p = fp_mul(a.c[i], b.c[j]);
      if (i + j < 4) r[i + j] = fp_add(r[i + j], p);
      else r[i + j - 4] = fp_add(r[i + j - 4], fp_mul(kNBeta, p));
    }
  return FpExt{{r[0], r[1], r[2], r[3]}};
}

// x^(p-2) by plain square-and-multiply
static uint32_t fp_inv_simple(uint32_t x) { return fp_pow(x, kP - 2); }

// fp_inv_batch<N> against fp_inv element by element; bit i of `zeros` puts a zero at position i
template <int N>
static void check_inv_batch(std::mt19937_64& rng, uint32_t zeros) {
  uint32_t x[N], want[N];
  for (int i = 0; i < N; i++) {
    x[i] = (zeros >> i) & 1 ? 0u : 1u + uint32_t(rng() % (kP - 1));
    want[i] = fp_inv(x[i]);
  }
  fp_inv_batch(x);
  for (int i = 0; i < N; i++)
    EXPECT(x[i] == want[i], "fp_inv_batch<%d> zeros=%#x position %d: %u, fp_inv gives %u\n", N, zeros, i, x[i], want[i]);
}

// zeros at: none; every single position; the first and last together; alternating (both
// phases); all positions
template <int N>
static void check_inv_batch_zero_patterns(std::mt19937_64& rng) {
  const uint32_t all = (1u << N) - 1u;
  for (int rep = 0; rep < 8; rep++) {
    check_inv_batch<N>(rng, 0);
    for (int i = 0; i < N; i++) check_inv_batch<N>(rng, 1u << i);
    check_inv_batch<N>(rng, 1u | (1u << (N - 1)));
    check_inv_batch<N>(rng, 0x55555555u & all);
    check_inv_batch<N>(rng, 0xaaaaaaaau & all);
    check_inv_batch<N>(rng, all);
  }
}

static void check_inverses(std::mt19937_64& rng, int n) {
  const uint32_t edge[] = {0, 1, kP - 1, kP - 2, kOne, kP - kOne};
  for (uint32_t x : edge) {
    EXPECT(fp_inv(x) == fp_inv_simple(x), "fp_inv(%u)\n", x);
    EXPECT(x == 0 ? fp_inv(x) == 0 : fp_mul(x, fp_inv(x)) == kOne, "x * fp_inv(x), x = %u\n", x);
  }
  for (int it = 0; it < n; it++) {
    const uint32_t x = uint32_t(rng() % kP);
    EXPECT(fp_inv(x) == fp_inv_simple(x), "fp_inv(%u)\n", x);
  }
  check_inv_batch_zero_patterns<1>(rng);
  check_inv_batch_zero_patterns<2>(rng);
  check_inv_batch_zero_patterns<8>(rng);
  check_inv_batch_zero_patterns<16>(rng);
  // fe_inv: 0 stays 0; x * fe_inv(x) = 1 on elements with one non-zero coefficient (edge and
  // random words in each position) and on random elements
  const FpExt z = fe_inv(fe_zero());
  EXPECT(fe_eq(z, fe_zero()), "fe_inv(0) = (%u, %u, %u, %u)\n", z.c[0], z.c[1], z.c[2], z.c[3]);
  for (int it = 0; it < 64; it++)
    for (int k = 0; k < 4; k++) {
      FpExt x = fe_zero();
      x.c[k] = it < 5 ? edge[it + 1] : 1u + uint32_t(rng() % (kP - 1));
      EXPECT(fe_eq(fe_mul(x, fe_inv(x)), fe_one()), "fe_inv, coefficient %d alone = %u\n", k, x.c[k]);
      if (k == 0) EXPECT(fe_inv(x).c[0] == fp_inv(x.c[0]), "fe_inv of a base-field word %u\n", x.c[0]);
    }
  for (int it = 0; it < 1000; it++) {
    FpExt x;
    for (int k = 0; k < 4; k++) x.c[k] = uint32_t(rng() % kP);
    EXPECT(fe_eq(x, fe_zero()) || fe_eq(fe_mul(x, fe_inv(x)), fe_one()), "fe_inv, random element it=%d\n", it);
  }
}

int main(int argc, char** argv) {
  int n = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::mt19937_64 rng(12345), inv_rng(54321);
  check_inverses(inv_rng, n < 2000 ? n : 2000);
  auto elem = [&](int mode) -> uint32_t {
    switch (mode) {
      case 0: return 0;
      case 1: return kP - 1;
      case 2: return kP - 1 - uint32_t(rng() % 8);
      default: return uint32_t(rng() % kP);
    }
  };
  for (int it = 0; it < n; it++) {
    int mode = it < 64 ? it % 4 : 3;
    uint32_t a[24], b[24];
    for (int i = 0; i < 24; i++) a[i] = b[i] = (it < 64 && (rng() & 1)) ? elem(mode) : elem(3);
    poseidon2_mix(a);
    poseidon2_mix_simple(b);
    for (int i = 0; i < 24; i++) EXPECT(a[i] == b[i], "poseidon2 mismatch it=%d cell=%d\n", it, i);
    // the signed full rounds read a word as int32: words in [p, 2^31) are still the right
    // value mod p (the tolerated range); the simple permutation gets their canonical form
    if (it < 2000) {
      for (int i = 0; i < 24; i++) {
        b[i] = uint32_t(rng() % kP);
        a[i] = (b[i] < 0x80000000u - kP && (rng() & 1)) ? b[i] + kP : b[i];
      }
      poseidon2_mix(a);
      poseidon2_mix_simple(b);
      for (int i = 0; i < 24; i++) EXPECT(a[i] == b[i], "poseidon2 [p, 2^31) input mismatch it=%d cell=%d\n", it, i);
    }
    FpExt x{{elem(mode), elem(3), elem(mode), elem(3)}}, y{{elem(3), elem(mode), elem(mode), elem(3)}};
    FpExt u = fe_mul(x, y), v = fe_mul_simple(x, y);
    for (int k = 0; k < 4; k++) EXPECT(u.c[k] == v.c[k], "fe_mul mismatch it=%d\n", it);
    uint64_t t = (uint64_t(rng()) >> 4);
    EXPECT(mont_reduce(fold64(t)) == mont_reduce(fold64(fold64(t))), "fold64 it=%d\n", it);
  }
  std::printf("%s (%d cases)\n", fails ? "FAIL" : "OK", n);
  return fails ? 1 : 0;
}
