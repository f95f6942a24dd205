// Poseidon2 over BabyBear, width 24 / rate 16 / 8 output cells, 4+21+4 rounds —
// the permutation of risc0/zkp/src/core/hash/poseidon2/mod.rs:102-216 with the
// parameters of poseidon2/consts.rs (Montgomery-encoded by tools/extract_poseidon2.py).
// Host+device: the device hashes Merkle rows/nodes, the host driver uses the same
// code for the Fiat-Shamir transcript (Poseidon2Rng, poseidon2/rng.rs:50-89).
#pragma once
#include "bb31.h"
#include "poseidon2_consts.inc"

namespace r0 {

#if defined(__HIP_DEVICE_COMPILE__)
__constant__ static const uint32_t kP2Full[8 * 24] = P2_FULL_RC_MONT;
__constant__ static const uint32_t kP2Partial[21] = P2_PARTIAL_RC_MONT;
__constant__ static const uint32_t kP2Diag[24] = P2_DIAG_MONT;
#else
static const uint32_t kP2Full[8 * 24] = P2_FULL_RC_MONT;
static const uint32_t kP2Partial[21] = P2_PARTIAL_RC_MONT;
static const uint32_t kP2Diag[24] = P2_DIAG_MONT;
#endif

// ---- reference formulation (mod.rs:102-216 step by step, every value canonical) ----
R0_HD uint32_t p2_sbox(uint32_t x) {
  uint32_t x2 = fp_mul(x, x);
  uint32_t x4 = fp_mul(x2, x2);
  uint32_t x6 = fp_mul(x4, x2);
  return fp_mul(x6, x);
}

// 4x4 circulant block of M_EXT (Poseidon2 paper, appendix B): mod.rs:137-148
R0_HD void p2_m4(uint32_t* x) {
  uint32_t t0 = fp_add(x[0], x[1]);
  uint32_t t1 = fp_add(x[2], x[3]);
  uint32_t t2 = fp_add(fp_add(x[1], x[1]), t1);
  uint32_t t3 = fp_add(fp_add(x[3], x[3]), t0);
  uint32_t t1_2 = fp_add(t1, t1), t0_2 = fp_add(t0, t0);
  uint32_t t4 = fp_add(fp_add(t1_2, t1_2), t3);
  uint32_t t5 = fp_add(fp_add(t0_2, t0_2), t2);
  uint32_t t6 = fp_add(t3, t5);
  uint32_t t7 = fp_add(t2, t4);
  x[0] = t6;
  x[1] = t5;
  x[2] = t7;
  x[3] = t4;
}

// M_EXT: mod.rs:150-173
R0_HD void p2_m_ext(uint32_t* c) {
  for (int i = 0; i < 6; i++) p2_m4(c + 4 * i);
  uint32_t s[4];
  for (int j = 0; j < 4; j++) {
    s[j] = fp_add(fp_add(fp_add(c[j], c[4 + j]), fp_add(c[8 + j], c[12 + j])), fp_add(c[16 + j], c[20 + j]));
  }
  for (int i = 0; i < 24; i++) c[i] = fp_add(c[i], s[i & 3]);
}

// M_INT = 1 + diag: mod.rs:129-135
R0_HD void p2_m_int(uint32_t* c) {
  uint32_t sum = 0;
  for (int i = 0; i < 24; i++) sum = fp_add(sum, c[i]);
  for (int i = 0; i < 24; i++) c[i] = fp_add(sum, fp_mul(kP2Diag[i], c[i]));
}

R0_HD void p2_full_round(uint32_t* c, int r) {
  for (int i = 0; i < 24; i++) c[i] = p2_sbox(fp_add(c[i], kP2Full[r * 24 + i]));
  p2_m_ext(c);
}

R0_HD void poseidon2_mix_simple(uint32_t* c) {
  p2_m_ext(c);
  for (int r = 0; r < 4; r++) p2_full_round(c, r);
  for (int r = 0; r < 21; r++) {
    c[0] = p2_sbox(fp_add(c[0], kP2Partial[r]));
    p2_m_int(c);
  }
  for (int r = 4; r < 8; r++) p2_full_round(c, r);
}

// ---- VALU-lean formulation (same permutation, ~30% fewer instructions) ----------
// Poseidon2 is integer-VALU bound on CDNA4 (one v_* per 4 cycles per SIMD), so the
// count of instructions is the cost. Bounds (p < 2^31):
//  * sbox: x^2 canonical, then three REDCs without the final umin: each product has
//    one factor < p and one < 2p, so t < 2p^2 < p*2^32 and the result is < 2p;
//  * M_EXT runs in 64-bit on those lazy (< 2p) cells: every output is a combination
//    with coefficient sum <= 112, so y < 224p < 2^39; the next round constant is
//    added in 64-bit and one lazy REDC feeds the S-box (scaled rounds, below);
//  * M_INT: c_i*d_i + S = REDC(c_i*d_i + S*2^32) and S*2^32 is congruent to
//    fold64(sum c_i * (2^32 mod p)) < 2^60, so multiply, add and reduce are one
//    v_mad_u64_u32 plus one REDC (t < p^2 + 2^60 < p*2^32).
R0_HD uint32_t p2_red39(uint64_t y) {
  uint32_t q = uint32_t((uint64_t(uint32_t(y >> 7)) * 273u) >> 32);
  uint32_t r = uint32_t(y) - q * kP;  // in [0, 2p)
  return umin(r, r - kP);
}
R0_HD uint32_t mont_lazy(uint64_t t) {  // t < p*2^32 -> t*2^-32 mod p in [0, 2p)
  uint32_t m = uint32_t(t) * kNegPinv;
  return uint32_t((t + uint64_t(m) * kP) >> 32);
}
// acc + a * b as one v_mad_u64_u32. Written as inline asm on the device so LLVM keeps
// the multiply-accumulate: for sum(c_i * C) it otherwise factors C out and sums the
// zero-extended c_i with a v_mov + v_lshl_add_u64 pair per cell.
R0_HD uint64_t mad64(uint32_t a, uint32_t b, uint64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(P2_NO_ASM)
  uint64_t r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "v"(b), "v"(acc));
  return r;
#else
  return uint64_t(a) * b + acc;
#endif
}
R0_HD uint32_t p2_sbox_lazy(uint32_t x) {  // x canonical -> x^7 in [0, 2p)
  uint32_t x2 = fp_mul(x, x);
  uint32_t x4 = mont_lazy(uint64_t(x2) * x2);
  uint32_t x6 = mont_lazy(uint64_t(x4) * x2);
  return mont_lazy(uint64_t(x6) * x);
}
// y = M_EXT * x over the integers (x < 2p). The 32-bit cells enter the 64-bit sums
// through v_mad_u64_u32 (x * 1 + acc, x * 2 + acc): a plain zero-extended add costs a
// v_mov of the high word per cell first (49 per round in p2_fold_kernel).
R0_HD void p2_m_ext64(const uint32_t* x, uint64_t* y) {
#pragma unroll
  for (int b = 0; b < 6; b++) {
    const uint32_t* v = x + 4 * b;
    uint64_t t0 = mad64(v[0], 1u, mad64(v[1], 1u, 0));
    uint64_t t1 = mad64(v[2], 1u, mad64(v[3], 1u, 0));
    uint64_t t2 = mad64(v[1], 2u, t1);
    uint64_t t3 = mad64(v[3], 2u, t0);
    uint64_t t4 = (t1 << 2) + t3;
    uint64_t t5 = (t0 << 2) + t2;
    y[4 * b] = t3 + t5;
    y[4 * b + 1] = t5;
    y[4 * b + 2] = t2 + t4;
    y[4 * b + 3] = t4;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint64_t s = ((y[j] + y[4 + j]) + (y[8 + j] + y[12 + j])) + (y[16 + j] + y[20 + j]);
#pragma unroll
    for (int b = 0; b < 6; b++) y[4 * b + j] += s;
  }
}

// ---- signed Montgomery for the full rounds -----------------------------------------
// Values are int32 in (-p, p). sredc(t) = (t - m p) / 2^32 with m = t * p^-1 mod 2^32 taken
// signed, so |result| < |t| / 2^32 + p/2: a product of two values below p in magnitude
// comes back below 0.969p, closed under multiplication with no correction step (the
// unsigned REDC needs a canonical square before x^4). Overflow bound: |t| + 2^31 p < 2^63,
// i.e. |t| < 1.2 p^2, which every product below keeps (bounds at each use). Same R^-1 per
// reduction as mont_lazy, so the scaled round constants of P2Scaled apply unchanged.
constexpr uint32_t kPinv = 0u - kNegPinv;  // p^-1 mod 2^32
R0_HD int64_t smad64(int32_t a, int32_t b, int64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(P2_NO_ASM)
  int64_t r;
  uint64_t carry;
  asm("v_mad_i64_i32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "v"(b), "v"(acc));
  return r;
#else
  return int64_t(a) * b + acc;
#endif
}
R0_HD int32_t sredc(int64_t t) {
  const int32_t m = int32_t(uint32_t(uint64_t(t)) * kPinv);
  return int32_t(uint64_t(t - int64_t(m) * int64_t(kP)) >> 32);  // low word is 0: exact
}
R0_HD int32_t smul(int32_t a, int32_t b) { return sredc(int64_t(a) * b); }
// |x| < 0.5p + 60 (after sredc of an M_EXT output) or x canonical: x^7 with every
// intermediate below 0.969p in magnitude (products at most 0.94 p^2). The partial rounds
// feed it up to 0.75p (p2b_sbox evaluates the same chain of bounds at compile time).
R0_HD int32_t p2_sbox_s(int32_t x) {
  const int32_t x2 = smul(x, x);
  const int32_t x4 = smul(x2, x2);
  const int32_t x6 = smul(x4, x2);
  return smul(x6, x);
}
R0_HD uint32_t s_canon(int32_t r) {  // (-p, p) -> [0, p)
  const uint32_t u = uint32_t(r);
  return umin(u, u + kP);
}
// y = M_EXT x over the integers, signed (|x| < 0.969p: |y| < 112 * 0.969p < 2^37)
R0_HD void p2_m_ext64s(const int32_t* x, int64_t* y) {
#pragma unroll
  for (int b = 0; b < 6; b++) {
    const int32_t* v = x + 4 * b;
    int64_t t0 = smad64(v[0], 1, smad64(v[1], 1, 0));
    int64_t t1 = smad64(v[2], 1, smad64(v[3], 1, 0));
    int64_t t2 = smad64(v[1], 2, t1);
    int64_t t3 = smad64(v[3], 2, t0);
    int64_t t4 = int64_t(uint64_t(t1) << 2) + t3;
    int64_t t5 = int64_t(uint64_t(t0) << 2) + t2;
    y[4 * b] = t3 + t5;
    y[4 * b + 1] = t5;
    y[4 * b + 2] = t2 + t4;
    y[4 * b + 3] = t4;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int64_t s = ((y[j] + y[4 + j]) + (y[8 + j] + y[12 + j])) + (y[16 + j] + y[20 + j]);
#pragma unroll
    for (int b = 0; b < 6; b++) y[4 * b + j] += s;
  }
}

// Full rounds without Barrett steps. A full round's M_EXT output y (< 224p + p with the
// next round constant) goes straight into a lazy REDC, which returns y * 2^-32 mod p in
// [0, p + 106) in two instructions instead of p2_red39's seven; that is small enough for
// the S-box's first Montgomery square. The REDC leaves the state scaled by 2^-32, so in
// round r the stored cells are X * sigma_r (X the true value, R = 2^32 mod p):
//   sigma_{r+1} = (sigma_r R^-1)^7 R^-6      (one REDC, then the S-box's four)
// and the round constants are stored pre-multiplied by sigma_r R^-1. One Montgomery
// multiply by R^3 / sigma restores the Montgomery form (X * R) before the partial rounds
// and at the end. Rounds 0 and 5 start from sigma = R, so their constants are unchanged.
//
// The constant enters the REDC's low word (round 6): with rcs = rc + (2^32 mod p) mod p (p if
// that is 0), sredc(y + rcs - 2^32) is congruent to sredc(y + rc), and its REDC multiplier
// m = lo(y + rcs - 2^32) p^-1 = (lo(y) + rcs) p^-1 needs only the 32-bit sum. The result is
// then exactly hi(y - m p): the low word of y - m p is 2^32 - rcs (the REDC zeroes the low word
// of y + rcs - 2^32 - m p), so adding rcs - 2^32 carries out and cancels. One full-rate
// v_add_u32 replaces the 64-bit add of rc per cell (sredc_rc). |y + rcs - 2^32| < 110.6p, so
// the output stays below 0.5p + 52.
//
// poseidon2_mix does not restore the Montgomery form in the middle: p2_partial_rounds (below)
// maps a state scaled by sigma_4 to one scaled by sigma_4, so its rounds 4-7 continue the
// chain from sigma_4 (rcs[96..191], k_end_s). poseidon2_mix_quad restores it (k_mid) and
// restarts round 5 from sigma = R (rc, k_end).
struct P2Scaled {
  uint32_t rc[8 * 24];   // rounds 0-3 and 5-7 restarted from R (round 4 uses kP2Full as it is)
  uint32_t k_mid, k_end;
  uint32_t rcs[8 * 24];  // rc + (2^32 mod p) mod p, in [1, p], for sredc_rc; rounds 4-7 continue from sigma_4
  uint32_t sigma_mid;    // sigma_4
  uint32_t k_end_s;      // R^3 / sigma_8 of the continued chain
};
constexpr uint32_t p2c_mul(uint32_t a, uint32_t b) { return uint32_t(uint64_t(a) * b % kP); }
constexpr uint32_t p2c_pow(uint32_t a, uint64_t e) {
  uint32_t r = 1;
  while (e) {
    if (e & 1) r = p2c_mul(r, a);
    a = p2c_mul(a, a);
    e >>= 1;
  }
  return r;
}
constexpr P2Scaled p2_make_scaled() {
  P2Scaled t{};
  const uint32_t full[8 * 24] = P2_FULL_RC_MONT;
  const uint32_t R = uint32_t((uint64_t(1) << 32) % kP), Rinv = p2c_pow(R, kP - 2);
  const uint32_t R3 = p2c_pow(R, 3), Rm6 = p2c_pow(Rinv, 6);
  for (int half = 0; half < 2; half++) {
    const int r0 = half ? 5 : 0, r1 = half ? 8 : 4;
    uint32_t sigma = R;
    for (int r = r0; r < r1; r++) {
      const uint32_t s = p2c_mul(sigma, Rinv);
      for (int i = 0; i < 24; i++) t.rc[r * 24 + i] = p2c_mul(full[r * 24 + i], s);
      sigma = p2c_mul(p2c_pow(s, 7), Rm6);
    }
    const uint32_t k = p2c_mul(R3, p2c_pow(sigma, kP - 2));
    if (half) t.k_end = k;
    else t.k_mid = k, t.sigma_mid = sigma;
  }
  for (int i = 0; i < 24; i++) t.rc[4 * 24 + i] = full[4 * 24 + i];
  for (int i = 0; i < 4 * 24; i++) {
    const uint32_t v = uint32_t((uint64_t(t.rc[i]) + R) % kP);
    t.rcs[i] = v ? v : kP;
  }
  uint32_t sigma = t.sigma_mid;
  for (int r = 4; r < 8; r++) {
    const uint32_t s = p2c_mul(sigma, Rinv);
    for (int i = 0; i < 24; i++) {
      const uint32_t v = uint32_t((uint64_t(p2c_mul(full[r * 24 + i], s)) + R) % kP);
      t.rcs[r * 24 + i] = v ? v : kP;
    }
    sigma = p2c_mul(p2c_pow(s, 7), Rm6);
  }
  t.k_end_s = p2c_mul(R3, p2c_pow(sigma, kP - 2));
  return t;
}
// sredc(y + rc) (mod p) for the stored round constant rcs = rc + (2^32 mod p): above
R0_HD int32_t sredc_rc(int64_t y, uint32_t rcs) {
  const int32_t m = int32_t((uint32_t(uint64_t(y)) + rcs) * kPinv);
  return int32_t(uint64_t(y - int64_t(m) * int64_t(kP)) >> 32);
}
#if defined(__HIP_DEVICE_COMPILE__)
__constant__ static const P2Scaled kP2S = p2_make_scaled();
#else
static constexpr P2Scaled kP2S = p2_make_scaled();
#endif

// ---- partial rounds as a block-linear map -------------------------------------------
// Only cell 0 passes the S-box and M_INT = J + diag(d) is linear, so the 23 passive cells
// stay untouched over a block of K = 7 rounds. With v_1..v_23 the cells at the block's
// start, u_j the S-box output of round j and S_j the cell sum M_INT adds in round j:
//   S_j     = u_j + sum_i d_i^j v_i + sum_{l<j} D_{j-1-l} S_l     (D_m = sum_{i>=1} d_i^m)
//   z_{j+1} = S_j + d_0 u_j + rc_{j+1}                            (next S-box input)
//   c_i     = d_i^K v_i + sum_{l<K} d_i^{K-1-l} S_l  (i >= 1),  c_0 = S_{K-1} + d_0 u_{K-1}
// Every product is a 32-bit value times a compile-time constant centred into (-p/2, p/2],
// accumulated in 64 bits: about 28 mads, three folds and two REDCs per round, and 8 mads, a
// fold and a REDC per cell per block, where the round-by-round form spends 48 mads and 24
// REDCs per round.
//
// Scales: the block takes and returns the passive cells as 64-bit values y_i = X_i sigma
// (sigma = sigma_4, whatever the full rounds left; it only enters the constants), reads them
// as v_i = sredc(y_i) = X_i sigma / R, and keeps z, u and s_j = sredc(..) = S_j R in
// Montgomery form, so the S-box needs no scaling and all three blocks share their constants.
// The last block's y feed round 4's sredc_rc directly.
//
// Bounds: sfold brings any int64 to at most 2^59 in magnitude (hi * (2^32 mod p) + lo), after
// which sredc returns below 2^27 + p/2 + 1 = 0.567p. An accumulator is folded before its
// worst case, the sum of |constant| * |input bound| over its terms, can pass 2^63, and
// before every sredc. P2PartialBounds evaluates each worst case from the actual constants;
// the static_asserts below it are the proof.
constexpr int kP2K = 7;                       // rounds per block
constexpr int kP2Seg0 = 9, kP2Seg1 = 18;      // an S_j row folds before v_9 and before v_18
constexpr int32_t p2c_centre(uint32_t a) { return a > kP / 2 ? int32_t(a - kP) : int32_t(a); }
struct P2Partial {
  int32_t ct[24][kP2K + 1];  // S_j row: ct[i][j] = d_i^j R^2 / sigma' on v_i (sigma' = sigma / R; row 0 and [i][K] unused)
  int32_t co[24][kP2K + 1];  // output row of cell i: co[i][m] = d_i^m sigma' on s_{K-1-m}, co[i][K] = d_i^K R on v_i
  int32_t cd[kP2K - 1];      // D_m R on s_{j-1-m}
  int32_t cu;                // R on u_j
  int32_t cz;                // d_0 R on u_j, for z_{j+1}
  int32_t k_in;              // R^2 / sigma': v_0 -> z_0
  int32_t k_out;             // sigma': z -> y_0 after the last block
  uint32_t rcz[22];          // rc_r R + (2^32 mod p) mod p in [1, p] for sredc_rc; [21] adds nothing
};
constexpr P2Partial p2_make_partial() {
  P2Partial t{};
  const uint32_t diag[24] = P2_DIAG_MONT, prc[21] = P2_PARTIAL_RC_MONT;
  const uint32_t R = uint32_t((uint64_t(1) << 32) % kP), Rinv = p2c_pow(R, kP - 2);
  const uint32_t sp = p2c_mul(p2_make_scaled().sigma_mid, Rinv), spinv = p2c_pow(sp, kP - 2);
  const uint32_t R2sp = p2c_mul(p2c_mul(R, R), spinv);
  uint32_t D[kP2K] = {};
  for (int i = 1; i < 24; i++) {
    const uint32_t d = p2c_mul(diag[i], Rinv);
    uint32_t dm = 1;  // d^m
    for (int m = 0; m <= kP2K; m++) {
      if (m < kP2K) {
        t.ct[i][m] = p2c_centre(p2c_mul(dm, R2sp));
        t.co[i][m] = p2c_centre(p2c_mul(dm, sp));
        D[m] = (D[m] + dm) % kP;
      } else {
        t.co[i][m] = p2c_centre(p2c_mul(dm, R));
      }
      dm = p2c_mul(dm, d);
    }
  }
  for (int m = 0; m < kP2K - 1; m++) t.cd[m] = p2c_centre(p2c_mul(D[m], R));
  t.cu = p2c_centre(R);
  t.cz = p2c_centre(diag[0]);
  t.k_in = p2c_centre(R2sp);
  t.k_out = p2c_centre(sp);
  for (int r = 0; r < 22; r++) {
    const uint32_t v = uint32_t((uint64_t(r < 21 ? p2c_mul(prc[r], R) : 0u) + R) % kP);
    t.rcz[r] = v ? v : kP;
  }
  return t;
}
#if defined(__HIP_DEVICE_COMPILE__)
__constant__ static const P2Partial kP2L = p2_make_partial();
#else
static constexpr P2Partial kP2L = p2_make_partial();
#endif

// acc + a * c for a constant c. The constant is a scalar operand (an SGPR the compiler fills
// with s_mov or s_load; smad64 would spend a v_mov per constant to put it in a VGPR). The
// unused carry goes to vcc: an SGPR pair of its own per mad crowds out the constants.
R0_HD int64_t smadc(int32_t a, int32_t c, int64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(P2_NO_ASM)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(a), "s"(c), "v"(acc) : "vcc");
  return r;
#else
  return int64_t(a) * c + acc;
#endif
}
R0_HD int64_t smulc(int32_t a, int32_t c) {  // a * c: the same mad with the inline constant 0
#if defined(__HIP_DEVICE_COMPILE__) && !defined(P2_NO_ASM)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(a), "s"(c) : "vcc");
  return r;
#else
  return int64_t(a) * c;
#endif
}
// hi * (2^32 mod p) + lo with hi signed and lo unsigned: congruent to t, at most 2^59 in magnitude
constexpr int32_t kFoldCs = int32_t(kFoldC);
R0_HD int64_t sfold(int64_t t) {
  return smadc(int32_t(uint32_t(uint64_t(t) >> 32)), kFoldCs, int64_t(uint64_t(uint32_t(uint64_t(t)))));
}

constexpr uint64_t kSredcMax = (uint64_t(1) << 63) - (uint64_t(kP) << 31) - 1;  // sredc: |t| + 2^31 p < 2^63
constexpr uint64_t kAccMax = (uint64_t(1) << 63) - 1;
constexpr uint64_t kSfoldOut = (uint64_t(1) << 31) * kFoldC + (uint64_t(1) << 32);  // |sfold(t)| <= this = 2^59
constexpr uint64_t kP2YIn = uint64_t(1) << 38;  // |y| entering the partial rounds: M_EXT of |x| < 2^31, 112 * 2^31
constexpr uint64_t p2b_add(uint64_t a, uint64_t b) { return a + b < a ? ~uint64_t(0) : a + b; }  // saturating
constexpr uint64_t p2b_abs(int32_t c) { return c < 0 ? uint64_t(-int64_t(c)) : uint64_t(c); }
constexpr uint64_t p2b_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
// |sredc(t)| for |t| <= T: (|t| + 2^31 p) / 2^32, rounded up; everything if sredc's own limit is passed
constexpr uint64_t p2b_sredc(uint64_t T) {
  return T > kSredcMax ? ~uint64_t(0) : ((T + (uint64_t(kP) << 31)) >> 32) + 1;
}
constexpr uint64_t p2b_smul(uint64_t a, uint64_t b) {
  return (a >> 32) || (b >> 32) ? ~uint64_t(0) : p2b_sredc(a * b);
}
constexpr uint64_t p2b_sbox(uint64_t x) {  // |p2_sbox_s(x)| for |x| <= x
  const uint64_t x2 = p2b_smul(x, x), x4 = p2b_smul(x2, x2), x6 = p2b_smul(x4, x2);
  return p2b_smul(x6, x);
}
struct P2PartialBounds {
  uint64_t v, s, u, z;  // |v_i|, |s_j|, |u_j|, |z_j| (as int32 values)
  uint64_t u_next;      // the bound on u that follows from u: at most u (the invariant)
  uint64_t acc;         // largest accumulator before a fold
  uint64_t redc;        // largest argument of a REDC
  uint64_t y0;          // |y_0| leaving the last block
};
constexpr P2PartialBounds p2_partial_bounds() {
  const P2Partial t = p2_make_partial();
  P2PartialBounds b{};
  b.v = p2b_sredc(p2b_max(kP2YIn, kSfoldOut));
  b.s = p2b_sredc(kSfoldOut);
  // z = sredc_rc(sfold(..) + u cz, rcz) and u = sbox(z): u <= p holds first (z_0 below) and is kept
  const uint64_t z_from_p = p2b_sredc(kSfoldOut + uint64_t(kP) * p2b_abs(t.cz) + (uint64_t(1) << 32));
  const uint64_t z0_arg = b.v * p2b_abs(t.k_in) + (uint64_t(1) << 32);
  b.u = p2b_max(p2b_sbox(z_from_p), p2b_sbox(p2b_sredc(z0_arg)));
  b.redc = p2b_max(kSfoldOut + b.u * p2b_abs(t.cz) + (uint64_t(1) << 32), z0_arg);  // z_{j+1} and z_0
  b.z = p2b_max(p2b_sredc(kSfoldOut + b.u * p2b_abs(t.cz) + (uint64_t(1) << 32)), p2b_sredc(z0_arg));
  b.u_next = p2b_sbox(b.z);
  for (int j = 0; j < kP2K; j++) {
    uint64_t a = 0;
    for (int i = 1; i < 24; i++) {
      if (i == kP2Seg0 || i == kP2Seg1) b.acc = p2b_max(b.acc, a), a = kSfoldOut;
      a = p2b_add(a, p2b_abs(t.ct[i][j]) * b.v);
    }
    for (int l = 0; l < j; l++) a = p2b_add(a, p2b_abs(t.cd[j - 1 - l]) * b.s);
    a = p2b_add(a, p2b_abs(t.cu) * b.u);
    b.acc = p2b_max(b.acc, a);
  }
  for (int i = 1; i < 24; i++) {
    uint64_t a = p2b_abs(t.co[i][kP2K]) * b.v;
    for (int m = 0; m < kP2K; m++) a = p2b_add(a, p2b_abs(t.co[i][m]) * b.s);
    b.acc = p2b_max(b.acc, a);
  }
  b.y0 = b.z * p2b_abs(t.k_out);
  return b;
}
constexpr P2PartialBounds kP2LB = p2_partial_bounds();
static_assert(kP2LB.v < (uint64_t(1) << 31) && kP2LB.s < (uint64_t(1) << 31), "v_i and s_j fit int32");
static_assert(kP2LB.u <= kP && kP2LB.u_next <= kP2LB.u, "|u| <= kP2LB.u is kept from round to round");
static_assert(kP2LB.z < (uint64_t(1) << 31) && p2b_sbox(kP2LB.z) <= kP, "z fits the S-box");
static_assert(kP2LB.acc <= kAccMax, "no accumulator passes 2^63 before its fold");
static_assert(kP2LB.redc <= kSredcMax && kSfoldOut <= kSredcMax, "every REDC argument is within sredc's limit");
// round 4 reads the last block's y through sredc_rc (rcs <= p < 2^32) and p2_sbox_s
static_assert(p2b_sbox(p2b_sredc(p2b_max(kP2LB.y0, kSfoldOut) + (uint64_t(1) << 32))) <= kP, "round 4 input");

// y[24]: the state times sigma (mod p), |y_i| <= 2^38 -> the state 21 partial rounds later,
// times sigma, |y_i| <= max(kSfoldOut, kP2LB.y0) < 2^61
R0_HD void p2_partial_rounds(int64_t* y) {
  int32_t v[24], s[kP2K];
  int32_t z = sredc_rc(smulc(sredc(y[0]), kP2L.k_in), kP2L.rcz[0]);
#pragma unroll 1
  for (int b = 0; b < 21 / kP2K; b++) {
    // Read the block's constants at an offset (0) the compiler cannot see through: loads
    // from a known __constant__ address are hoisted out of this loop and the caller's, and
    // ~200 hoisted constants spill from SGPRs to VGPR lanes (a v_readlane per use).
    uint32_t o = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(o));
#endif
    const P2Partial* t = &kP2L + o;
#pragma unroll
    for (int i = 1; i < 24; i++) v[i] = sredc(y[i]);
    // the passive cells' share of every S_j first, cell by cell: seven independent chains
    // (a v_mad_i64_i32 that reads the one before it waits a cycle) and one run of constants per cell
    int64_t a[kP2K];
#pragma unroll
    for (int i = 1; i < 24; i++) {
#pragma unroll
      for (int j = 0; j < kP2K; j++) {
        if (i == kP2Seg0 || i == kP2Seg1) a[j] = sfold(a[j]);
        a[j] = i == 1 ? smulc(v[i], t->ct[i][j]) : smadc(v[i], t->ct[i][j], a[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kP2K; j++) {
      const int32_t u = p2_sbox_s(z);
      int64_t f = a[j];
#pragma unroll
      for (int l = 0; l < j; l++) f = smadc(s[l], t->cd[j - 1 - l], f);
      f = sfold(smadc(u, t->cu, f));
      s[j] = sredc(f);
      z = sredc_rc(smadc(u, t->cz, f), t->rcz[b * kP2K + j + 1]);
    }
#pragma unroll
    for (int i = 1; i < 24; i += 2) {  // two cells' chains interleaved
      const int i1 = i + 1 < 24 ? i + 1 : i;
      int64_t f0 = smulc(v[i], t->co[i][kP2K]), f1 = smulc(v[i1], t->co[i1][kP2K]);
#pragma unroll
      for (int l = 0; l < kP2K; l++) {
        f0 = smadc(s[l], t->co[i][kP2K - 1 - l], f0);
        if (i1 != i) f1 = smadc(s[l], t->co[i1][kP2K - 1 - l], f1);
      }
      y[i] = sfold(f0);
      if (i1 != i) y[i1] = sfold(f1);
    }
  }
  y[0] = smulc(z, kP2L.k_out);  // rcz[21] added nothing: z is cell 0 in Montgomery form
}

R0_HD void poseidon2_mix(uint32_t* c) {
  int64_t y[24];
  int32_t x[24];
#pragma unroll
  for (int i = 0; i < 24; i++) x[i] = int32_t(c[i]);  // canonical: below p < 2^31
  p2_m_ext64s(x, y);
  // Full rounds in signed Montgomery (above): |y + rc| < 113p, so sredc returns below
  // 0.5p + 54, the S-box's input. Rolled: each round's 24 constants are loaded at the top
  // of its iteration instead of all 168 living in SGPRs (which spill to VGPR lanes in
  // hash_rows).
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 24; i++) x[i] = p2_sbox_s(sredc_rc(y[i], kP2S.rcs[r * 24 + i]));
    p2_m_ext64s(x, y);
  }
  // The partial rounds keep the scale sigma_4 (p2_partial_rounds), so rounds 4-7 go on as
  // rounds 1-3 do, with constants scaled along the continued chain; round 4's input is
  // below 0.57p in magnitude (static_assert above), within the S-box's range.
  p2_partial_rounds(y);
#pragma unroll 1
  for (int r = 4; r < 8; r++) {
#pragma unroll
    for (int i = 0; i < 24; i++) x[i] = p2_sbox_s(sredc_rc(y[i], kP2S.rcs[r * 24 + i]));
    p2_m_ext64s(x, y);
  }
#pragma unroll
  for (int i = 0; i < 24; i++) c[i] = s_canon(smul(sredc(y[i]), int32_t(kP2S.k_end_s)));
}

#if defined(__HIP__)
// ---- one permutation over a lane quad (wavefront-shuffle formulation) -------------
// Lane q = lane & 3 of a quad holds cells 4j + q (j = 0..5): position q of every 4x4 block
// of M_EXT. The block mix needs the other three positions of the block (three DPP
// quad_perm moves per block, no LDS); the block sum s[q] of M_EXT and the per-cell
// M_INT diagonal are lane-local; the M_INT sum over all 24 cells is a two-step quad
// all-reduce. Same arithmetic and bounds as poseidon2_mix, so the words are identical.
// About 2.6k VALU instructions per lane against 7.6k for one lane per permutation: a
// third of the latency for 1.4x the issued work, so it pays only where a layer leaves
// SIMDs idle (Merkle tree tops), not in the throughput-bound leaf and layer hashing.
__device__ __forceinline__ uint32_t p2q_dpp(uint32_t v, int sel) {
  switch (sel) {  // quad_perm lane selectors for q^1, q^2, q^3
    case 1: return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0xB1, 0xF, 0xF, false));
    case 2: return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0x4E, 0xF, 0xF, false));
    default: return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0x1B, 0xF, 0xF, false));
  }
}
__device__ __forceinline__ uint64_t p2q_dpp64(uint64_t v, int sel) {
  return (uint64_t(p2q_dpp(uint32_t(v >> 32), sel)) << 32) | p2q_dpp(uint32_t(v), sel);
}
// M4 rows (p2_m4 as a matrix): [5 7 1 3] [4 6 1 1] [1 3 5 7] [1 1 4 6]; m[d] = M4[q][q ^ d]
struct P2Quad {
  uint32_t m[4];
  uint32_t q;
  __device__ __forceinline__ explicit P2Quad(uint32_t lane) : q(lane & 3) {
    constexpr uint32_t M4[16] = {5, 7, 1, 3, 4, 6, 1, 1, 1, 3, 5, 7, 1, 1, 4, 6};
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t qq = 0; qq < 4; qq++) v = q == qq ? M4[qq * 4 + (qq ^ d)] : v;
      m[d] = v;
    }
  }
  // y = M_EXT x over the integers for this lane's six cells (x < 2p)
  __device__ __forceinline__ void m_ext(const uint32_t* x, uint64_t* y) const {
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      uint64_t t = uint64_t(x[j]) * m[0];
      t = mad64(p2q_dpp(x[j], 1), m[1], t);
      t = mad64(p2q_dpp(x[j], 2), m[2], t);
      t = mad64(p2q_dpp(x[j], 3), m[3], t);
      y[j] = t;
      s += t;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) y[j] += s;
  }
};

__device__ __forceinline__ void poseidon2_mix_quad(uint32_t* c) {
  const P2Quad Q(threadIdx.x);
  const uint32_t q = Q.q;
  uint64_t y[6];
  uint32_t x[6];
  Q.m_ext(c, y);
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int j = 0; j < 6; j++) x[j] = p2_sbox_lazy(mont_lazy(y[j] + kP2S.rc[r * 24 + 4 * j + q]));
    Q.m_ext(x, y);
  }
#pragma unroll
  for (int j = 0; j < 6; j++) c[j] = fp_mul(mont_lazy(y[j]), kP2S.k_mid);
  uint32_t diag[6];
#pragma unroll
  for (int j = 0; j < 6; j++) diag[j] = kP2Diag[4 * j + q];
#pragma unroll 1
  for (int r = 0; r < 21; r++) {
    const uint32_t u = p2_sbox_lazy(fp_add(umin(c[0], c[0] - kP), kP2Partial[r]));
    c[0] = q == 0 ? u : c[0];  // cell 0 lives in lane 0 of the quad
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) s = mad64(c[j], kFoldC, s);
    s = fold64(s);
    s += p2q_dpp64(s, 1);
    s += p2q_dpp64(s, 2);
    const uint64_t sf = fold64(s);
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = mont_lazy(uint64_t(c[j]) * diag[j] + sf);
  }
#pragma unroll
  for (int j = 0; j < 6; j++) c[j] = umin(c[j], c[j] - kP);
#pragma unroll
  for (int j = 0; j < 6; j++) x[j] = p2_sbox_lazy(fp_add(c[j], kP2Full[4 * 24 + 4 * j + q]));
  Q.m_ext(x, y);
#pragma unroll 1
  for (int r = 5; r < 8; r++) {
#pragma unroll
    for (int j = 0; j < 6; j++) x[j] = p2_sbox_lazy(mont_lazy(y[j] + kP2S.rc[r * 24 + 4 * j + q]));
    Q.m_ext(x, y);
  }
#pragma unroll
  for (int j = 0; j < 6; j++) c[j] = fp_mul(mont_lazy(y[j]), kP2S.k_end);
}
#endif

}  // namespace r0
