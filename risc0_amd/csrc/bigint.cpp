// rv32im BigInt accumulation states: the first half of the witness generator's accum step.
//
// Before the per-cycle accumulation runs, the reference computes, with the final mix drawn
// from the transcript, the running BigInt accumulator state (poly, term, total: three FpExt)
// after every Back::BigInt cycle of the preflight trace, and scatters those 12 words into
// accum columns 0..11 of the cycle's row
// (circuit/rv32im/src/prove/witgen/mod.rs:178-205; BigIntAccum::{new,step},
// witgen/byte_poly.rs:381-470; offsets :362-377). The generated step code then reads the
// previous cycle's state at back 1 (rv32im.accum.ir), which is why it must be in place before
// the step kernels run on all cycles at once.
//
// The reference runs the recurrence as a serial host loop, and so does
// rv32im_bigint_accum_states below (r0hip_rv32im_bigint_accum_states; no GPU needed). A
// segment of an RSA, ECDSA or pairing guest is BigInt cycles almost end to end, and the loop
// then takes longer than the rest of the proof, between the mix draw and the accum commit
// where nothing else of that proof can be queued. So the provers take the device path,
// rv32im_bigint_accum_states_device: the integer checks on the records (rows inside the
// segment and strictly increasing, poly_op in range) stay a host pass that finds the first
// structurally bad record ks; records [0, ks) are uploaded as they are and their states come
// from three parallel scans (bigint_accum.hip), which also find the first failing EqZero; one
// word is read back, and the earliest failure in trace order is reported with the serial
// loop's message. rv32im_bigint_inject scatters the states from device memory (accum.hip),
// taking the row of each record from the uploaded records. Below kDeviceMinRecords records
// the serial loop with an upload of its states is faster and is kept (DESIGN.md section 4 has
// the measurement).
#include <string>
#include <vector>

#include "../../include/r0hip.h"
#include "bb31.h"
#include "runtime.h"

namespace r0 {

namespace {
constexpr int kWidthBytes = 16;  // BIGINT_WIDTH_BYTES (risc0_circuit_rv32im::execute::bigint)
constexpr size_t kMixWords = 36; // REGCOUNT_MIX
constexpr uint32_t kOps = 7;     // PolyOp (bigint.rs:62-70)
// rv32im_bigint_inject: the device path from this many records on (profiles/r7_bigint_accum.json)
constexpr size_t kDeviceMinRecords = 4096;

FpExt fe_u32(uint32_t v) { return fe_from_fp(fp_encode(v)); }  // ExtVal::from_u32

// The integer checks of record k, in the serial loop's order; what fails, or nothing.
bool record_ok(const r0hip_bigint_back* backs, size_t k, size_t rows) {
  return backs[k].row < rows && (k == 0 || backs[k].row > backs[k - 1].row) && backs[k].poly_op < kOps;
}
void require_record(const r0hip_bigint_back* backs, size_t k, size_t rows) {
  const r0hip_bigint_back& b = backs[k];
  R0_REQUIRE(b.row < rows, "bigint back: row " + std::to_string(b.row) + " outside the segment");
  R0_REQUIRE(k == 0 || b.row > backs[k - 1].row, "bigint backs must be in increasing row order (trace order)");
  R0_REQUIRE(b.poly_op < kOps, "bigint back: invalid poly_op " + std::to_string(b.poly_op));
}
std::string eqz_message(uint32_t row) { return "Invalid eqz in bigint accum (row " + std::to_string(row) + ")"; }
}  // namespace

// byte_poly.rs:381-470, restated over this library's field code; one state per record
std::vector<uint32_t> rv32im_bigint_accum_states(const uint32_t* mix, const r0hip_bigint_back* backs, size_t n,
                                                 size_t rows) {
  // the final mix (witgen/mod.rs:184: mix[mix.len() - 4..])
  const FpExt last_mix{{mix[kMixWords - 4], mix[kMixWords - 3], mix[kMixWords - 2], mix[kMixWords - 1]}};
  FpExt powers[kWidthBytes + 1];  // MAX_POWERS = BIGINT_WIDTH_BYTES + 1
  FpExt cur = fe_one();
  for (auto& p : powers) {
    p = cur;
    cur = fe_mul(cur, last_mix);
  }
  FpExt neg_poly = fe_zero();
  for (int i = 0; i < kWidthBytes; i++) neg_poly = fe_add(neg_poly, fe_mul(powers[i], fe_u32(128)));
  FpExt poly = fe_zero(), term = fe_one(), total = fe_zero();  // BigIntAccumState::new
  auto reset = [&] {
    poly = fe_zero();
    term = fe_one();
    total = fe_zero();
  };
  std::vector<uint32_t> out(n * 12);
  for (size_t k = 0; k < n; k++) {
    const r0hip_bigint_back& b = backs[k];
    if (!record_ok(backs, k, rows)) require_record(backs, k, rows);
    FpExt delta = fe_zero();
    for (int i = 0; i < kWidthBytes; i++) delta = fe_add(delta, fe_mul(powers[i], fe_u32(b.bytes[i])));
    const FpExt new_poly = fe_add(poly, delta);
    switch (b.poly_op) {
      case 0:  // Reset
        reset();
        break;
      case 1:  // Shift
        poly = fe_mul(new_poly, powers[kWidthBytes]);
        break;
      case 2:  // SetTerm
        poly = fe_zero();
        term = new_poly;
        break;
      case 3: {  // AddTotal
        const FpExt coeff = fe_sub(fe_u32(b.coeff), fe_u32(4));
        total = fe_add(total, fe_mul(fe_mul(coeff, term), new_poly));
        poly = fe_zero();
        term = fe_one();
        break;
      }
      case 4:  // Carry1
        poly = fe_add(poly, fe_mul(fe_sub(delta, neg_poly), fe_u32(64 * 256)));
        break;
      case 5:  // Carry2
        poly = fe_add(poly, fe_mul(delta, fe_u32(256)));
        break;
      default: {  // 6, EqZero
        const FpExt carry = fe_sub(powers[1], fe_u32(256));
        const FpExt goal = fe_add(total, fe_mul(new_poly, carry));
        R0_REQUIRE(fe_eq(goal, fe_zero()), eqz_message(b.row));
        reset();
        break;
      }
    }
    // BigIntAccumState::as_array order: poly, term, total (offsets 0..11)
    for (int i = 0; i < 4; i++) {
      out[k * 12 + i] = poly.c[i];
      out[k * 12 + 4 + i] = term.c[i];
      out[k * 12 + 8 + i] = total.c[i];
    }
  }
  return out;
}

const r0hip_bigint_back* rv32im_bigint_accum_states_device(hipStream_t s, uint32_t* d_states, const uint32_t* mix,
                                                           const r0hip_bigint_back* backs, size_t n, size_t rows) {
  R0_REQUIRE(rows <= (size_t(1) << 26), "bigint accum: rows above 2^26");
  // the first record that fails an integer check; an EqZero before it fails first
  size_t ks = 0;
  while (ks < n && record_ok(backs, ks, rows)) ks++;
  const r0hip_bigint_back* d_backs = nullptr;
  if (ks) {
    auto* up = static_cast<r0hip_bigint_back*>(scratch(ks * sizeof(r0hip_bigint_back), kSlotBigIntBacks));
    uint32_t* d_fail = static_cast<uint32_t*>(scratch(4, kSlotBigIntFail));
    upload_async(up, backs, ks * sizeof(r0hip_bigint_back));
    bigint_accum_scan(s, d_states, up, ks, mix, d_fail);
    uint32_t fail = 0;
    download(&fail, d_fail, 4);
    if (fail < ks) R0_REQUIRE(false, eqz_message(backs[fail].row));
    d_backs = up;
  }
  if (ks < n) require_record(backs, ks, rows);
  return d_backs;
}

// the injection itself: the states, then one lane per record writes its 12 words
void rv32im_bigint_inject(hipStream_t s, uint32_t* accum, size_t rows, const uint32_t* mix,
                          const r0hip_bigint_back* backs, size_t n) {
  if (n == 0) return;
  R0_REQUIRE(backs, "bigint backs: null pointer with a nonzero count");
  uint32_t* d_states = static_cast<uint32_t*>(scratch(n * 48, kSlotBigIntStates));
  if (n >= kDeviceMinRecords) {
    const r0hip_bigint_back* d_backs = rv32im_bigint_accum_states_device(s, d_states, mix, backs, n, rows);
    bigint_scatter(s, accum, rows, reinterpret_cast<const uint32_t*>(d_backs), d_states, n,
                   sizeof(r0hip_bigint_back) / 4);
    return;
  }
  std::vector<uint32_t> states = rv32im_bigint_accum_states(mix, backs, n, rows);
  std::vector<uint32_t> row_of(n);
  for (size_t k = 0; k < n; k++) row_of[k] = backs[k].row;
  uint32_t* d_rows = static_cast<uint32_t*>(scratch(n * 4, kSlotBigIntRows));
  upload_async(d_rows, row_of.data(), n * 4);
  upload_async(d_states, states.data(), n * 48);
  bigint_scatter(s, accum, rows, d_rows, d_states, n);
}

}  // namespace r0
