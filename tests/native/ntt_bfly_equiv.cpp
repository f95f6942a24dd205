// Host check of risc0_amd/csrc/ntt_bfly.h: the range-typed helpers against 128-bit
// reference arithmetic with every documented output range asserted, and bfly_group (the
// code ntt.hip's stage_group runs) word for word against the same network written with the
// canonical fp_add / fp_sub / fp_mul. R0_NTT_BFLY_CHECK compiles the header's own range
// assertions in: no addend ever sees a word >= p.
//   usage: ntt_bfly_equiv [random cases, default 1000000]
#define R0_NTT_BFLY_CHECK 1
#include "ntt_bfly.h"

#include <stdio.h>
#include <stdlib.h>

using namespace r0;
typedef unsigned __int128 u128;

static uint64_t g_state = 0x5249534330ull;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static uint32_t rnd_fp() { return uint32_t(rnd64() % kP); }

static int g_fail = 0;
#define CHECK(c, ...)                        \
  do {                                       \
    if (!(c)) {                              \
      if (g_fail++ < 20) {                   \
        printf("FAIL %s: ", #c);             \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

// ---- helpers ------------------------------------------------------------------------
static uint64_t g_rinv;  // 2^-32 mod p

static uint64_t pow_mod(uint64_t b, uint64_t e) {
  u128 r = 1, x = b % kP;
  for (; e; e >>= 1, x = x * x % kP)
    if (e & 1) r = r * x % kP;
  return uint64_t(r);
}

static void check_mul(uint32_t y, uint32_t w) {
  const uint64_t want = uint64_t(u128(y) * w % kP * g_rinv % kP);
  const uint32_t lazy = fp_mul_wide_lazy(y, w), full = fp_mul_wide(y, w);
  CHECK(lazy < 2 * uint64_t(kP) && lazy % kP == want, "fp_mul_wide_lazy(%u, %u) = %u, want %llu mod p", y, w, lazy,
        (unsigned long long)want);
  CHECK(full == want, "fp_mul_wide(%u, %u) = %u, want %llu", y, w, full, (unsigned long long)want);
  // a lazy product is a valid first operand of the next one
  const uint32_t chain = fp_mul_wide(lazy, w);
  CHECK(chain == uint64_t(u128(want) * w % kP * g_rinv % kP), "chain through a lazy product (%u, %u)", y, w);
  if (y < kP) CHECK(full == fp_mul(y, w), "fp_mul_wide(%u, %u) differs from fp_mul", y, w);
}

static void check_addsub(uint32_t a, uint32_t b) {
  const uint32_t s = fp_add_lazy(a, b), d = fp_sub_lazy(a, b);
  CHECK(s < 2 * uint64_t(kP) && s % kP == (uint64_t(a) + b) % kP, "fp_add_lazy(%u, %u) = %u", a, b, s);
  CHECK(d >= 1 && d < 2 * uint64_t(kP) && d % kP == (uint64_t(a) + kP - b) % kP, "fp_sub_lazy(%u, %u) = %u", a, b, d);
  CHECK(s % kP == fp_add(a, b) && d % kP == fp_sub(a, b), "lazy add/sub of (%u, %u) against fp_add/fp_sub", a, b);
}

static void test_helpers(long nrand) {
  g_rinv = pow_mod((uint64_t(1) << 32) % kP, kP - 2);
  const uint32_t ys[] = {0, 1, kP - 1, kP, kP + 1, 2 * kP - 1, 0x80000000u, 0xffffffffu};
  const uint32_t ws[] = {0, 1, 2, kP - 2, kP - 1};
  for (uint32_t y : ys)
    for (uint32_t w : ws) check_mul(y, w);
  for (uint32_t a : ws)
    for (uint32_t b : ws) check_addsub(a, b);
  for (long i = 0; i < nrand; i++) {
    check_mul(uint32_t(rnd64()), rnd_fp());
    check_addsub(rnd_fp(), rnd_fp());
  }
}

// ---- the group network --------------------------------------------------------------
// twiddles of one group: t[st][q], q < 2^st
struct Tw {
  uint32_t t[3][4];
  uint32_t operator()(uint32_t st, uint32_t q) const { return t[st][q]; }
};

// stage_group's loops as they were with canonical helpers only
template <int NST, bool INV, bool TRIV>
static void ref_group(uint32_t (&v)[1 << NST], const Tw& tw) {
  constexpr uint32_t M = 1u << NST;
  if (!INV) {
    for (uint32_t st = 0; st < NST; st++) {
      const uint32_t half = 1u << st;
      for (uint32_t m = 0; m < M; m++) {
        if (m & half) continue;
        uint32_t x = v[m], y = v[m + half];
        if (!(TRIV && (m & (half - 1)) == 0)) y = fp_mul(y, tw(st, m & (half - 1)));
        v[m] = fp_add(x, y);
        v[m + half] = fp_sub(x, y);
      }
    }
  } else {
    for (int st = NST - 1; st >= 0; st--) {
      const uint32_t half = 1u << st;
      for (uint32_t m = 0; m < M; m++) {
        if (m & half) continue;
        uint32_t x = v[m], y = v[m + half];
        v[m] = fp_add(x, y);
        v[m + half] = fp_sub(x, y);
        if (!(TRIV && (m & (half - 1)) == 0)) v[m + half] = fp_mul(v[m + half], tw(uint32_t(st), m & (half - 1)));
      }
    }
  }
}

template <int NST, bool INV, bool TRIV>
static void one_case(const uint32_t* in, const Tw& tw) {
  constexpr uint32_t M = 1u << NST;
  uint32_t a[M], b[M];
  for (uint32_t m = 0; m < M; m++) a[m] = b[m] = in[m];
  bfly_group<NST, INV, TRIV>(a, tw);
  ref_group<NST, INV, TRIV>(b, tw);
  for (uint32_t m = 0; m < M; m++)
    CHECK(a[m] == b[m], "NST %d INV %d TRIV %d: v[%u] = %u, want %u (in[0] %u, tw[0][0] %u)", NST, int(INV),
          int(TRIV), m, a[m], b[m], in[0], tw.t[0][0]);
}

static Tw tw_fill(uint32_t w) {
  Tw t;
  for (auto& s : t.t)
    for (auto& x : s) x = w;
  return t;
}
static Tw tw_random() {
  Tw t;
  for (auto& s : t.t)
    for (auto& x : s) x = rnd_fp();
  return t;
}

template <int NST, bool INV, bool TRIV>
static void test_group(long nrand) {
  constexpr uint32_t M = 1u << NST;
  // all p-1, all 1 (the plain word and the Montgomery word of one), three random tables
  const Tw fixed[] = {tw_fill(kP - 1), tw_fill(1), tw_fill(kOne), tw_random(), tw_random(), tw_random()};
  uint32_t v[M];
  for (const Tw& tw : fixed) {
    // every assignment of {0, p-1} to the 2^NST positions: all 0, all p-1, (p-1, 0)
    // alternating with every period and in every phase, a single p-1 (and a single 0) at
    // each position
    for (uint32_t mask = 0; mask < (1u << M); mask++) {
      for (uint32_t m = 0; m < M; m++) v[m] = (mask >> m & 1) ? kP - 1 : 0;
      one_case<NST, INV, TRIV>(v, tw);
    }
    // a single p-1 among random words, at each position
    for (uint32_t pos = 0; pos < M; pos++) {
      for (uint32_t m = 0; m < M; m++) v[m] = m == pos ? kP - 1 : rnd_fp();
      one_case<NST, INV, TRIV>(v, tw);
    }
  }
  for (long i = 0; i < nrand; i++) {
    for (uint32_t m = 0; m < M; m++) v[m] = rnd_fp();
    one_case<NST, INV, TRIV>(v, (i & 3) == 3 ? fixed[i >> 2 & 3] : tw_random());
  }
}

int main(int argc, char** argv) {
  const long nrand = argc > 1 ? atol(argv[1]) : 1000000;
  test_helpers(nrand);
  test_group<1, false, false>(nrand);
  test_group<1, false, true>(nrand);
  test_group<1, true, false>(nrand);
  test_group<1, true, true>(nrand);
  test_group<2, false, false>(nrand);
  test_group<2, false, true>(nrand);
  test_group<2, true, false>(nrand);
  test_group<2, true, true>(nrand);
  test_group<3, false, false>(nrand);
  test_group<3, false, true>(nrand);
  test_group<3, true, false>(nrand);
  test_group<3, true, true>(nrand);
  if (g_fail) {
    printf("FAILED: %d mismatches\n", g_fail);
    return 1;
  }
  printf("OK %ld random cases per helper and per network\n", nrand);
  return 0;
}
