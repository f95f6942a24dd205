// Host-side check of p2_partial_rounds (the 21 partial rounds as three block-linear maps)
// against 21 iterations of p2_sbox / p2_m_int on the canonical state, with inputs at the
// edges of its documented range (tests/test_p2_partial_host.py builds and runs this, once
// plain and once with -fsanitize=signed-integer-overflow,undefined).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "poseidon2.h"

using namespace r0;

static int fails = 0;
#define EXPECT(c, ...)                            \
  do {                                            \
    if (!(c)) {                                   \
      if (fails++ < 10) std::printf(__VA_ARGS__); \
    }                                             \
  } while (0)

static uint32_t mod_p(int64_t y) {
  const int64_t r = y % int64_t(kP);
  return uint32_t(r < 0 ? r + int64_t(kP) : r);
}

// y with sredc(y) at the top (sign > 0) or bottom (sign < 0) of its range for |y| <= 2^38:
// the low word is chosen so that the REDC multiplier is -2^31 or 2^31 - 1
static int64_t y_extreme(int sign) {
  if (sign > 0) return (int64_t(63) << 32) | int64_t(0x80000000u);
  const uint32_t lo = uint32_t(0x7fffffffu * uint64_t(kP));
  return -(int64_t(64) << 32) + int64_t(lo);
}

static int cases = 0;
static void check(const int64_t* y_in, const char* what, int idx) {
  const uint32_t R = uint32_t((uint64_t(1) << 32) % kP), Rinv = p2c_pow(R, kP - 2);
  const uint32_t sigma = kP2S.sigma_mid;
  const uint32_t to_mont = p2c_mul(R, p2c_pow(sigma, kP - 2));  // y -> Montgomery word
  const uint32_t from_mont = p2c_mul(sigma, Rinv);
  uint32_t c[24];
  int64_t y[24];
  for (int i = 0; i < 24; i++) {
    y[i] = y_in[i];
    c[i] = p2c_mul(mod_p(y[i]), to_mont);
  }
  for (int r = 0; r < 21; r++) {
    c[0] = p2_sbox(fp_add(c[0], kP2Partial[r]));
    p2_m_int(c);
  }
  p2_partial_rounds(y);
  const uint64_t out_max = p2b_max(kSfoldOut, kP2LB.y0);
  for (int i = 0; i < 24; i++) {
    EXPECT(mod_p(y[i]) == p2c_mul(c[i], from_mont), "%s %d: cell %d differs\n", what, idx, i);
    EXPECT(uint64_t(y[i] < 0 ? -y[i] : y[i]) <= out_max, "%s %d: cell %d out of range\n", what, idx, i);
  }
  cases++;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 4000;
  std::mt19937_64 rng(20240607);
  const int64_t ext[2] = {y_extreme(-1), y_extreme(+1)};
  // the extremes are what they claim: sredc at +-(p/2 + 63), within the bound the header proves
  EXPECT(sredc(ext[1]) >= int32_t(kP / 2) + 63 && uint64_t(sredc(ext[1])) <= kP2LB.v, "positive extreme %d\n", sredc(ext[1]));
  EXPECT(sredc(ext[0]) <= -int32_t(kP / 2) - 63 && uint64_t(-int64_t(sredc(ext[0]))) <= kP2LB.v, "negative extreme %d\n",
         sredc(ext[0]));
  auto rnd_y = [&]() -> int64_t { return int64_t(rng() % ((uint64_t(1) << 39) + 1)) - (int64_t(1) << 38); };

  int64_t y[24];
  for (int s = 0; s < 2; s++) {  // every cell at one extreme, and at the ends of the stated range
    for (int i = 0; i < 24; i++) y[i] = ext[s];
    check(y, "all-extreme", s);
    for (int i = 0; i < 24; i++) y[i] = s ? (int64_t(1) << 38) : -(int64_t(1) << 38);
    check(y, "range-end", s);
  }
  for (int i = 0; i < 24; i++) y[i] = 0;
  check(y, "zero", 0);
  // one case per S_j row and polarity: every v_i carries the sign of its constant (or the
  // opposite one), so the row's passive-cell sum is driven to its bound; cell 0 at both ends
  for (int j = 0; j < kP2K; j++)
    for (int pol = 0; pol < 2; pol++)
      for (int c0 = 0; c0 < 2; c0++) {
        y[0] = ext[c0];
        for (int i = 1; i < 24; i++) y[i] = ext[(kP2L.ct[i][j] >= 0) ^ pol];
        check(y, "S-row", j * 4 + pol * 2 + c0);
      }
  // one case per output row and polarity: v_i carries the sign of its own constant; the other
  // cells take the signs of the row of S_{K-1}, the sum with the largest weight in the output
  for (int i = 1; i < 24; i++)
    for (int pol = 0; pol < 2; pol++) {
      y[0] = ext[pol];
      for (int k = 1; k < 24; k++) y[k] = ext[(kP2L.ct[k][kP2K - 1] >= 0) ^ pol];
      y[i] = ext[(kP2L.co[i][kP2K] >= 0) ^ pol];
      check(y, "out-row", i * 2 + pol);
    }
  for (int it = 0; it < n; it++) {  // random states; a third of them with cells drawn from the extremes
    for (int i = 0; i < 24; i++) y[i] = (it % 3 == 0 && (rng() & 1)) ? ext[rng() & 1] : rnd_y();
    check(y, "random", it);
  }
  std::printf("%s (%d cases)\n", fails ? "FAIL" : "OK", cases);
  return fails ? 1 : 0;
}
