// Preflight::step on the host (recursion_preflight.h). Values are the reference's Montgomery
// words throughout (Fp holds them the same way), so the WOM and the IOP values are written in
// the form the witness generator reads, with no conversion pass.
#include "recursion_preflight.h"

#include <cstring>
#include <stdexcept>

#include "poseidon2.h"

namespace r0 {
namespace rpf {
namespace {

// control column offsets (CODE_LAYOUT, layout.rs.inc:224-330)
constexpr uint32_t kColWriteAddr = 0, kColMicro = 1, kColMacro = 2, kColP2Load = 3, kColP2Full = 4, kColP2Partial = 5,
                   kColP2Store = 6, kColCheckedBytes = 7, kColInst = 8;
constexpr uint32_t kColBitAndElem = 11, kColBitOpShorts = 12, kColShaInit = 13, kColShaFini = 14, kColShaLoad = 15,
                   kColShaMix = 16, kColMacroOperand = 18;
constexpr uint32_t kColP2Flags = 8, kColP2G1 = 13, kColP2G2 = 14, kColP2Inputs = 15;
// preflight.rs:36-37: 2^32 and 2^-32 mod p, multiplied in as Fp::from(u32)
constexpr uint32_t kToMont = fp_encode(0xFFFFFFEu), kFromMont = fp_encode(0x38400000u);
constexpr uint32_t kShiftWord = fp_encode(1u << 16);

inline uint32_t enc(uint32_t x) { return fp_mul(kR2, x); }        // Fp::new, x < p
inline uint32_t dec(uint32_t x) { return mont_reduce(x); }         // Fp::as_u32
inline uint32_t reduce(uint32_t x) {                               // x mod p for any u32 (2^32 < 3p)
  x = umin(x, x - kP);
  return umin(x, x - kP);
}

[[noreturn]] void refuse(const std::string& msg) { throw std::runtime_error("r0hip: recursion preflight: " + msg); }

// SHA-256 (FIPS 180-4): the initial state and the compression function, numeric words
constexpr uint32_t kShaInitState[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                       0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr uint32_t kShaK[64] = {
    0x428A2F98u, 0x71374491u, 0xB5C0FBCFu, 0xE9B5DBA5u, 0x3956C25Bu, 0x59F111F1u, 0x923F82A4u, 0xAB1C5ED5u,
    0xD807AA98u, 0x12835B01u, 0x243185BEu, 0x550C7DC3u, 0x72BE5D74u, 0x80DEB1FEu, 0x9BDC06A7u, 0xC19BF174u,
    0xE49B69C1u, 0xEFBE4786u, 0x0FC19DC6u, 0x240CA1CCu, 0x2DE92C6Fu, 0x4A7484AAu, 0x5CB0A9DCu, 0x76F988DAu,
    0x983E5152u, 0xA831C66Du, 0xB00327C8u, 0xBF597FC7u, 0xC6E00BF3u, 0xD5A79147u, 0x06CA6351u, 0x14292967u,
    0x27B70A85u, 0x2E1B2138u, 0x4D2C6DFCu, 0x53380D13u, 0x650A7354u, 0x766A0ABBu, 0x81C2C92Eu, 0x92722C85u,
    0xA2BFE8A1u, 0xA81A664Bu, 0xC24B8B70u, 0xC76C51A3u, 0xD192E819u, 0xD6990624u, 0xF40E3585u, 0x106AA070u,
    0x19A4C116u, 0x1E376C08u, 0x2748774Cu, 0x34B0BCB5u, 0x391C0CB3u, 0x4ED8AA4Au, 0x5B9CCA4Fu, 0x682E6FF3u,
    0x748F82EEu, 0x78A5636Fu, 0x84C87814u, 0x8CC70208u, 0x90BEFFFAu, 0xA4506CEBu, 0xBEF9A3F7u, 0xC67178F2u};
inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline uint32_t bswap(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24); }
void sha256_compress(uint32_t state[8], const uint32_t block[16]) {
  uint32_t w[64];
  for (int t = 0; t < 16; t++) w[t] = block[t];
  for (int t = 16; t < 64; t++)
    w[t] = w[t - 16] + (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] +
           (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10));
  uint32_t v[8];
  for (int i = 0; i < 8; i++) v[i] = state[i];
  for (int t = 0; t < 64; t++) {
    const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
                        kShaK[t] + w[t];
    const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
    for (int i = 7; i > 0; i--) v[i] = v[i - 1];
    v[4] += t1;
    v[0] = t1 + t2;
  }
  for (int i = 0; i < 8; i++) state[i] += v[i];
}

struct Decoder {
  Program p;
  uint64_t iops = 0, outputs = 0, wom = 0;
  uint32_t sha_init_pos = 0, sha_load_pos = 0, sha_fini_pos = 0;  // preflight.rs:71-73: the row order fixes them
  void wrote(uint32_t addr) {
    if (addr < p.wom_cap() && uint64_t(addr) + 1 > wom) wom = uint64_t(addr) + 1;
  }
  // w: the row's 23 words as plain integers below p
  void row(const uint32_t* w, size_t r) {
    Op op{};
    op.wa = w[kColWriteAddr];
    bool safe = false;
    const uint32_t iop_idx = uint32_t(iops);
    if (w[kColMacro] == 1) {
      op.kind = kMacro;
      for (int i = 0; i < 3; i++) op.arg[i] = w[kColMacroOperand + i];
      if (w[kColBitAndElem] == 1) op.sub[0] = kBitAndElem;
      else if (w[kColBitOpShorts] == 1) op.sub[0] = kBitOpShorts;
      else if (w[kColShaInit] == 1) {
        op.sub[0] = kShaInit;
        op.sub[1] = uint8_t(sha_init_pos);
        sha_init_pos = (sha_init_pos + 1) % 4;
      } else if (w[kColShaLoad] == 1) {
        op.sub[0] = kShaLoad;
        op.sub[1] = uint8_t(sha_load_pos);
        sha_load_pos = (sha_load_pos + 1) % 16;
      } else if (w[kColShaMix] == 1) {
        op.sub[0] = kShaMix;
      } else if (w[kColShaFini] == 1) {
        op.sub[0] = kShaFini;
        op.sub[1] = uint8_t(sha_fini_pos);
        // the first sha_fini of four writes the digest at args[0] - 3 .. + 4 (preflight.rs:465)
        if (sha_fini_pos == 0 && op.arg[0] >= 3)
          for (uint32_t i = 0; i < 8; i++) wrote(uint32_t((uint64_t(op.arg[0]) - 3 + i) % kP));
        sha_fini_pos = (sha_fini_pos + 1) % 4;
      }
      if (op.sub[0] == kBitAndElem || op.sub[0] == kBitOpShorts) wrote(op.wa);
      safe = op.sub[0] < kShaInit;  // the SHA rows are not parallel-safe
    } else if (w[kColMicro] == 1) {
      op.kind = kMicro;
      safe = true;
      for (uint32_t i = 0; i < 3; i++) {
        const uint32_t* m = w + kColInst + 4 * i;
        op.sub[i] = m[0] <= kExtract ? uint8_t(m[0]) : uint8_t(kUnknown);
        for (int k = 0; k < 3; k++) op.arg[3 * i + k] = m[1 + k];
        const uint32_t wa = uint32_t((uint64_t(op.wa) + i) % kP);
        switch (op.sub[i]) {
          case kEq: break;
          case kReadIopHeader: {
            const uint64_t count = m[1], k = m[2] / 2;
            p.n_input += k == 2 ? count : k * count;
            break;
          }
          case kUnknown: break;
          case kReadIopBody: iops++; wrote(wa); break;
          case kAdd: outputs += m[3] != 0; wrote(wa); break;
          case kMixRng: safe = safe && m[3] == 0; wrote(wa); break;
          default: wrote(wa);
        }
      }
    } else if (w[kColCheckedBytes] == 1) {
      refuse("row " + std::to_string(r) + " is a checked_bytes row, which no C++ witness generator runs "
             "(extern_readCoefficients is not implemented)");
    } else if (w[kColP2Load] == 1 || (w[kColP2Full] != 1 && w[kColP2Partial] != 1 && w[kColP2Store] == 1)) {
      // Preflight::step's order: load, full, partial, store (a row with two selectors takes the first)
      const bool load = w[kColP2Load] == 1;
      op.kind = load ? kP2Load : kP2Store;
      op.sub[0] = w[kColP2Flags] != 0 ? kFlagDoMont : 0;
      if (load) {
        op.sub[0] |= (w[kColP2Flags + 1] == 1 ? kFlagKeepState : 0) | (w[kColP2Flags + 2] == 1 ? kFlagKeepUpper : 0);
        for (int i = 0; i < 8; i++) op.arg[i] = w[kColP2Inputs + i];
      }
      const uint64_t group = uint64_t(w[kColP2G1]) + 2 * uint64_t(w[kColP2G2]);
      op.sub[1] = group < 3 ? uint8_t(group) : uint8_t(0xFF);
      if (!load && group < 3)
        for (uint32_t i = 0; i < 8; i++) wrote(uint32_t((uint64_t(op.wa) + i) % kP));
    } else if (w[kColP2Full] == 1) {
      op.kind = kP2Full;
    } else if (w[kColP2Partial] == 1) {
      op.kind = kP2Partial;
    } else {
      op.kind = kIllegal;
    }
    p.ops.push_back(op);
    p.cycles.push_back(iop_idx);
    p.cycles.push_back(safe ? 1u : 0u);
  }
  Program finish() {
    p.n_wom = size_t(wom);
    p.n_iops = size_t(iops);
    p.n_output = size_t(outputs);
    return std::move(p);
  }
};

void check_shape(size_t rows, uint32_t po2) {
  if (po2 < 11 || po2 > 24) refuse("po2 " + std::to_string(po2) + " outside 11..24");
  if (rows == 0) refuse("the program has no rows");
  if (rows > (size_t(1) << po2) - kZkCycles)
    refuse(std::to_string(rows) + " rows, above 2^po2 - ZK_CYCLES = " + std::to_string((size_t(1) << po2) - kZkCycles));
}

struct Machine {
  const Program& p;
  const uint32_t* input;
  size_t n_input, in_pos = 0;
  uint32_t* wom;
  size_t wom_len = 0;
  uint32_t* iops;
  size_t n_iops = 0;
  uint32_t* output;
  size_t n_output = 0;
  uint32_t p2[24] = {};
  uint32_t sha_state[8] = {}, sha_load[16] = {};
  // the IOP body read by the last header: `count` polynomials of k input words from `base`
  // (k == 2: one word each, split into shorts), `next` the first unread one
  struct {
    size_t base = 0;
    uint64_t count = 0, k = 0, next = 0;
    bool flip = false;
  } body;
  size_t cycle = 0;

  [[noreturn]] void fail(const std::string& msg) const {
    throw std::runtime_error("r0hip: recursion preflight: " + msg + " (cycle " + std::to_string(cycle) + ")");
  }
  static std::string show(FpExt v) {
    return "[" + std::to_string(dec(v.c[0])) + ", " + std::to_string(dec(v.c[1])) + ", " + std::to_string(dec(v.c[2])) +
           ", " + std::to_string(dec(v.c[3])) + "]";
  }
  void check_addr(uint32_t addr) const {
    if (addr >= p.wom_cap())
      fail("WOM address " + std::to_string(addr) + " at or above the library's cap of 16 * 2^po2 = " +
           std::to_string(p.wom_cap()) + " cells");
  }
  FpExt wom_read(uint32_t addr) const {
    check_addr(addr);
    if (addr >= wom_len)
      fail("WOM read of address " + std::to_string(addr) + " past the memory's " + std::to_string(wom_len) + " cells");
    FpExt v;
    memcpy(v.c, wom + size_t(addr) * 4, 16);
    return v;
  }
  void wom_write(uint32_t addr, FpExt val) {
    check_addr(addr);  // below the cap, so below n_wom (decode counted every write address)
    if (wom_len <= addr) wom_len = size_t(addr) + 1;
    FpExt cur;
    memcpy(cur.c, wom + size_t(addr) * 4, 16);
    if (!fe_eq(cur, fe_zero()) && !fe_eq(cur, val))
      fail("WOM " + std::to_string(addr) + " overwritten with " + show(val) + " from " + show(cur));
    memcpy(wom + size_t(addr) * 4, val.c, 16);
  }

  void micro(uint8_t opcode, const uint32_t* a, uint32_t wa) {
    switch (opcode) {
      case kConst: wom_write(wa, FpExt{{enc(a[0]), enc(a[1]), 0, 0}}); break;
      case kAdd: {
        const FpExt x = wom_read(a[0]), y = wom_read(a[1]);
        wom_write(wa, fe_add(x, y));
        if (a[2] != 0) output[n_output++] = dec(x.c[0]);
        break;
      }
      case kSub: {
        const FpExt x = wom_read(a[0]), y = wom_read(a[1]);
        wom_write(wa, fe_sub(x, y));
        break;
      }
      case kMul: {
        const FpExt x = wom_read(a[0]), y = wom_read(a[1]);
        wom_write(wa, fe_mul(x, y));
        break;
      }
      case kInv: {
        const FpExt x = wom_read(a[0]);
        wom_write(wa, a[1] == 0 ? fe_from_fp(x.c[0] == 0 ? kOne : 0u) : fe_inv(x));
        break;
      }
      case kEq: {
        const FpExt x = wom_read(a[0]), y = wom_read(a[1]);
        if (!fe_eq(x, y)) fail("Equality check failed: Expecting " + show(x) + " == " + show(y));
        break;
      }
      case kReadIopHeader: {
        if (body.next < body.count)
          fail("READ_IOP_HEADER while the IOP body has " + std::to_string(body.count - body.next) + " unread values");
        const uint64_t count = a[0], k = a[1] / 2;
        const uint64_t need = k == 2 ? count : k * count;  // below 2^62
        if (need > n_input - in_pos)
          fail("input exhausted: READ_IOP_HEADER reads " + std::to_string(need) + " words, " +
               std::to_string(n_input - in_pos) + " left");
        body.base = in_pos;
        body.count = count;
        body.k = k;
        body.next = 0;
        body.flip = (a[1] & 1) == 1;
        in_pos += size_t(need);
        break;
      }
      case kReadIopBody: {
        if (body.next >= body.count) fail("READ_IOP_BODY on an empty IOP body");
        const uint64_t i = body.next++;
        FpExt v = fe_zero();
        if (body.k == 2) {
          const uint32_t e = input[body.base + i];
          v.c[0] = enc(e & 0xFFFFu);
          v.c[1] = enc(e >> 16);
        } else {
          for (uint64_t j = 0; j < body.k && j < 4; j++)  // Fp::new_raw: the word is the Montgomery form
            v.c[j] = reduce(input[body.base + (body.flip ? i * body.k + j : j * body.count + i)]);
        }
        if (a[2] != 0) v = fe_mul_fp(v, kToMont);
        wom_write(wa, v);
        memcpy(iops + 4 * n_iops++, v.c, 16);
        break;
      }
      case kMixRng: {
        uint32_t val = enc(a[2]);
        if (a[2] != 0) val = fp_mul(val, wom_read(wa == 0 ? kP - 1 : wa - 1).c[0]);
        const FpExt x = wom_read(a[0]), y = wom_read(a[1]);
        val = fp_add(fp_mul(val, kShiftWord), x.c[1]);
        val = fp_add(fp_mul(val, kShiftWord), x.c[0]);
        val = fp_add(fp_mul(val, kShiftWord), y.c[1]);
        val = fp_add(fp_mul(val, kShiftWord), y.c[0]);
        wom_write(wa, fe_from_fp(val));
        break;
      }
      case kSelect: {
        const FpExt x = wom_read(a[0]);
        const uint32_t addr = uint32_t((uint64_t(a[1]) + uint64_t(a[2]) * dec(x.c[0])) % kP);
        wom_write(wa, wom_read(addr));
        break;
      }
      case kExtract: {
        const FpExt x = wom_read(a[0]);
        const uint32_t a1 = enc(a[1]), a2 = enc(a[2]), n1 = fp_sub(kOne, a1), n2 = fp_sub(kOne, a2);
        const uint32_t v = fp_add(fp_add(fp_mul(fp_mul(a1, a2), x.c[3]), fp_mul(fp_mul(a1, n2), x.c[2])),
                                  fp_add(fp_mul(fp_mul(n1, a2), x.c[1]), fp_mul(fp_mul(n1, n2), x.c[0])));
        wom_write(wa, fe_from_fp(v));
        break;
      }
      default: fail("Unknown opcode");
    }
  }

  void step(const Op& op) {
    switch (op.kind) {
      case kMacro:
        if (op.sub[0] == kBitAndElem) {
          const FpExt x = wom_read(op.arg[0]), y = wom_read(op.arg[1]);
          wom_write(op.wa, fe_from_fp(enc(dec(x.c[0]) & dec(y.c[0]))));
        } else if (op.sub[0] == kBitOpShorts) {
          const FpExt x = wom_read(op.arg[0]), y = wom_read(op.arg[1]);
          const uint32_t x0 = dec(x.c[0]), x1 = dec(x.c[1]), y0 = dec(y.c[0]), y1 = dec(y.c[1]);
          if (op.arg[2] != 0)  // Fp::new of the u32 sum (wrapping as the release build does)
            wom_write(op.wa, fe_from_fp(enc(reduce((x0 & y0) + ((x1 & y1) << 16)))));
          else
            wom_write(op.wa, FpExt{{enc(reduce(x0 ^ y0)), enc(reduce(x1 ^ y1)), 0, 0}});
        } else if (op.sub[0] == kShaInit) {
          if (op.sub[1] == 0)
            for (int i = 0; i < 8; i++) sha_state[i] = kShaInitState[i];
        } else if (op.sub[0] == kShaLoad) {
          // subtype 0: the element's Montgomery word (as_u32_montgomery); else two shorts
          const FpExt x = wom_read(op.arg[0]);
          sha_load[op.sub[1]] = op.arg[2] == 0 ? x.c[0] : dec(x.c[0]) + (dec(x.c[1]) << 16);
        } else if (op.sub[0] == kShaFini && op.sub[1] == 0) {
          // the loaded words are the block's bytes in memory order; the digest goes out the same way
          if (op.arg[0] < 3) fail("sha_fini: the output address args[0] - 3 is below zero");
          uint32_t block[16];
          for (int i = 0; i < 16; i++) block[i] = bswap(sha_load[i]);
          sha256_compress(sha_state, block);
          for (uint32_t i = 0; i < 8; i++) {
            const uint32_t out = bswap(sha_state[i]);
            wom_write(uint32_t((uint64_t(op.arg[0]) - 3 + i) % kP), FpExt{{enc(out & 0xFFFFu), enc(out >> 16), 0, 0}});
          }
        }
        break;
      case kMicro:
        for (uint32_t i = 0; i < 3; i++)
          micro(op.sub[i], op.arg + 3 * i, uint32_t((uint64_t(op.wa) + i) % kP));
        break;
      case kP2Load: {
        if (op.sub[1] > 2) fail("Poseidon2 load: group out of range");
        if (!(op.sub[0] & kFlagKeepState)) memset(p2, 0, (op.sub[0] & kFlagKeepUpper) ? 64 : 96);
        for (int i = 0; i < 8; i++) {
          uint32_t load = wom_read(op.arg[i]).c[0];
          if (op.sub[0] & kFlagDoMont) load = fp_mul(load, kFromMont);
          uint32_t& cell = p2[op.sub[1] * 8 + i];
          cell = fp_add(cell, load);
        }
        break;
      }
      case kP2Full: break;
      case kP2Partial: poseidon2_mix(p2); break;
      case kP2Store: {
        if (op.sub[1] > 2) fail("Poseidon2 store: group out of range");
        for (uint32_t i = 0; i < 8; i++) {
          uint32_t v = p2[op.sub[1] * 8 + i];
          if (op.sub[0] & kFlagDoMont) v = fp_mul(v, kToMont);
          wom_write(uint32_t((uint64_t(op.wa) + i) % kP), fe_from_fp(v));
        }
        break;
      }
      default: fail("Illegal recursion op");
    }
  }
};

}  // namespace

Program decode(const uint32_t* code, size_t n_words, int form, uint32_t po2) {
  if (!code) refuse("the code is NULL");
  if (form != 0 && form != 1) refuse("form " + std::to_string(form) + " is neither encoded (0) nor Montgomery (1)");
  if (n_words % kCodeCols != 0) refuse("n_words " + std::to_string(n_words) + " is not a multiple of 23 (words per row)");
  const size_t rows = n_words / kCodeCols;
  check_shape(rows, po2);
  Decoder d;
  d.p.po2 = po2;
  d.p.ops.reserve(rows);
  d.p.cycles.reserve(2 * rows);
  uint32_t w[kCodeCols];
  for (size_t r = 0; r < rows; r++) {
    for (uint32_t c = 0; c < kCodeCols; c++) {
      const uint32_t x = code[r * kCodeCols + c];
      if (form == 1 && x >= kP)
        refuse("code word " + std::to_string(r * kCodeCols + c) + " = " + std::to_string(x) +
               " is not a canonical Montgomery word (>= p)");
      w[c] = form == 1 ? dec(x) : reduce(x);
    }
    d.row(w, r);
  }
  return d.finish();
}

Program decode_columns(const uint32_t* ctrl, size_t rows, uint32_t po2) {
  if (!ctrl) refuse("the control group is NULL");
  check_shape(rows, po2);
  const size_t n = size_t(1) << po2;
  Decoder d;
  d.p.po2 = po2;
  d.p.ops.reserve(rows);
  d.p.cycles.reserve(2 * rows);
  uint32_t w[kCodeCols];
  for (size_t r = 0; r < rows; r++) {
    for (uint32_t c = 0; c < kCodeCols; c++) w[c] = dec(reduce(ctrl[c * n + r]));
    d.row(w, r);
  }
  return d.finish();
}

void run(const Program& p, const uint32_t* input, size_t n_input, uint32_t* wom, uint32_t* iops, uint32_t* output) {
  if ((n_input && !input) || (p.n_wom && !wom) || (p.n_iops && !iops) || (p.n_output && !output))
    refuse("null array with a nonzero count");
  if (p.n_wom) memset(wom, 0, p.n_wom * 16);
  Machine m{p, input, n_input, 0, wom, 0, iops, 0, output, 0, {}, {}, {}, {}, 0};
  for (size_t c = 0; c < p.ops.size(); c++) {
    m.cycle = c;
    m.step(p.ops[c]);
  }
}

}  // namespace rpf
}  // namespace r0
