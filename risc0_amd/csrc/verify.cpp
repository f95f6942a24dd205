// Host-side seal verifier: the STARK verifier of risc0-zkp, natively, so a host can check
// a seal from r0hip_prove_segment(s) before it leaves the process (the reference prover
// verifies its own receipts, zkvm/src/host/server/prove/prover_impl.rs:165-170).
//   verify            risc0/zkp/src/verify/mod.rs:500-560 (+ rv32im version word, circuit/rv32im/src/lib.rs:78-92)
//   groups            mod.rs:201-244
//   the rest          verify_core.h (read IOP, Merkle, verify_validity, FRI)
// Everything the reference checks is checked: transcript replay, the validity equation
// (mod.rs:340-394, with poly_ext run from the circuit's constraint program), every Merkle
// path, every FRI fold, the final polynomial and the seal length, plus the check_code hook
// (mod.rs:531): the code (control) root is returned, and when the caller passes an allow-list
// the root must be in it. Field words in the seal must be canonical (read_field_elem_slice).
// r0hip_testing_verify_seal_structure skips the validity equation for seals of synthetic
// witnesses, which do not satisfy the constraints; it is for tests, never for receipts.
// Host code only — no HIP call, so it runs without a GPU; the one exception is opt-in:
// r0hip_verify_seal_on(R0HIP_VERIFY_DEVICE, ...) hands the deferred Merkle openings to the device
// (device_openings below), everything else of the check staying here.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/r0hip.h"
#include "circuit.h"
#include "runtime.h"
#include "verify_core.h"

namespace r0 {

// r0hip_set_verify_device_poseidon254: whether a device check takes Poseidon254 openings too
static std::atomic<int> g_verify_device_p254{0};
bool verify_device_poseidon254() { return g_verify_device_p254.load(std::memory_order_relaxed) != 0; }

// PolyExt::poly_ext (the circuits' generated poly_ext.rs, e.g. circuit/recursion/src/poly_ext.rs,
// as called by verify_validity, zkp/src/verify/mod.rs:356-386): the constraint polynomial at
// the out-of-domain point from the tap evaluations, by running the circuit's flattened program
// (CircuitDef::ir, from <c>.poly.ir) over FpExt. mix/global are Montgomery words; eval_u holds
// one value per tap in tap order.
// The program run once: val[id] of every value, pows[k] of every poly_mix power; returns the id
// the `r` record names.
static uint32_t poly_ext_values(const CircuitDef& c, const uint32_t* mix, const uint32_t* global, const FpExt* eval_u,
                                FpExt poly_mix, std::vector<FpExt>& val, std::vector<FpExt>& pows) {
  pows.resize(c.n_poly_mix);
  for (size_t k = 0; k < c.n_poly_mix; k++) pows[k] = fe_pow(poly_mix, c.poly_mix_powers[k]);
  val.assign(c.n_ir, fe_zero());
  for (size_t k = 0; k < c.n_ir; k++) {
    const uint32_t* r = c.ir + 6 * k;
    FpExt& v = val[r[1]];
    switch (r[0]) {
      case 0: v = fe_from_fp(r[2]); break;                              // c: constant
      case 1: v = FpExt{{r[2], r[3], r[4], r[5]}}; break;               // e: extension constant
      case 2: v = eval_u[r[2]]; break;                                   // l: tap
      case 3: v = fe_from_fp((r[2] ? global : mix)[r[3]]); break;        // g: mix / global word
      case 4: v = fe_add(val[r[2]], val[r[3]]); break;
      case 5: v = fe_sub(val[r[2]], val[r[3]]); break;
      case 6: v = fe_mul(val[r[2]], val[r[3]]); break;
      case 7: v = fe_add(val[r[2]], fe_mul(val[r[3]], pows[r[4]])); break;  // a: acc + x * mix^k
      case 8: v = fe_add(val[r[2]], fe_mul(fe_mul(val[r[3]], val[r[4]]), pows[r[5]])); break;
      case 9: return r[1];  // r: result (the record names the value in its dst slot)
      default: throw std::runtime_error("r0hip: bad constraint program record");
    }
  }
  throw std::runtime_error("r0hip: constraint program has no result");
}

FpExt poly_ext(const CircuitDef& c, const uint32_t* mix, const uint32_t* global, const FpExt* eval_u,
               FpExt poly_mix) {
  std::vector<FpExt> val, pows;
  return val[poly_ext_values(c, mix, global, eval_u, poly_mix, val, pows)];
}

// Which term of the constraint program one trace row violates (r0hip_constraint_term). taps:
// the row's tap values, one base-field Montgomery word per tap in tap order. The accumulate
// chain that ends at the result (each `a`/`b` record's first operand is the chain's previous
// link) is walked in chain order, first link first, for the first link that adds a nonzero
// amount: x * mix^k for an `a`, x * y * mix^k for a `b`. An `a` is a single constraint and its
// id is the answer. A `b` is a guarded block: the walk repeats inside the operand that is
// itself an accumulate chain, and the innermost id found is the answer (the `b`'s own id when
// neither operand is a chain, or when no link inside adds anything). -1: no term is violated.
// The ids are those of the committed <circuit>.poly.ir.
int32_t constraint_term(const CircuitDef& c, const uint32_t* taps, const uint32_t* mix, const uint32_t* global,
                        FpExt poly_mix) {
  std::vector<FpExt> eval_u(c.n_taps);
  for (size_t i = 0; i < c.n_taps; i++) eval_u[i] = fe_from_fp(taps[i]);
  std::vector<FpExt> val, pows;
  const uint32_t res = poly_ext_values(c, mix, global, eval_u.data(), poly_mix, val, pows);
  std::vector<const uint32_t*> rec(c.n_ir, nullptr);  // by id
  for (size_t k = 0; k < c.n_ir; k++)
    if (c.ir[6 * k] != 9) rec[c.ir[6 * k + 1]] = c.ir + 6 * k;
  auto is_acc = [&](uint32_t id) { return rec[id] && (rec[id][0] == 7 || rec[id][0] == 8); };
  auto nonzero = [](FpExt v) { return (v.c[0] | v.c[1] | v.c[2] | v.c[3]) != 0; };
  // the first link of the chain ending at `end` that adds a nonzero amount, or -1
  auto first_link = [&](uint32_t end) -> int32_t {
    std::vector<uint32_t> chain;
    for (uint32_t id = end; is_acc(id); id = rec[id][2]) chain.push_back(id);
    for (size_t i = chain.size(); i-- > 0;) {
      const uint32_t* r = rec[chain[i]];
      const FpExt add = r[0] == 7 ? fe_mul(val[r[3]], pows[r[4]]) : fe_mul(fe_mul(val[r[3]], val[r[4]]), pows[r[5]]);
      if (nonzero(add)) return int32_t(chain[i]);
    }
    return -1;
  };
  int32_t term = first_link(res);
  while (term >= 0 && rec[term][0] == 8) {
    const uint32_t* r = rec[term];
    const int32_t inner = is_acc(r[3]) ? first_link(r[3]) : (is_acc(r[4]) ? first_link(r[4]) : -1);
    if (inner < 0) break;
    term = inner;
  }
  return term;
}

namespace {
using namespace vfy;

// The device opening backend (r0hip_verify_seal_on with R0HIP_VERIFY_DEVICE): the pending list as
// an r0hip_opening table over the seal words, hashed by merkle_open_host on the calling thread's
// stream. The launcher checks every range again and refuses on the host. Suite 2 gets here only
// when verify_entry_on found the Poseidon254 switch on, so it is allowed here without a second read.
void device_openings(int suite, const uint32_t* words, size_t n_words, const std::vector<PendingOpening>& pending,
                     OpeningResult* out) {
  const size_t n = pending.size();
  std::vector<r0hip_opening> table(n);
  for (size_t i = 0; i < n; i++) {
    const PendingOpening& p = pending[i];
    table[i].row_off = uint64_t(p.row - words);
    table[i].path_off = uint64_t(p.path - words);
    table[i].index = uint64_t(p.idx) + p.tree->rows;
    R0_REQUIRE(p.tree->cols <= kMerkleOpenMaxCols, "merkle_open: a group of " + std::to_string(p.tree->cols) +
                                                       " columns is wider than the device openings take");
    table[i].cols = uint32_t(p.tree->cols);
    table[i].levels = uint32_t(p.tree->path_levels(p.idx));
  }
  std::vector<uint32_t> digests(n * 8), status(n);
  merkle_open_host(suite, words, n_words, table.data(), n, digests.data(), status.data(), /*allow_p254=*/true);
  for (size_t i = 0; i < n; i++) {
    out[i].cur = digest_of(&digests[8 * i]);
    out[i].status = status[i];
  }
}

uint32_t verify_seal(const CircuitDef& c, int suite, const uint32_t* seal, size_t len, bool check_validity,
                     const uint32_t* code_roots, size_t n_code_roots, uint32_t* code_root_out,
                     OpeningBackend backend = nullptr) {
  if (c.name == std::string("rv32im")) {  // rv32im/src/lib.rs:78-92: a version word leads the seal
    if (len < 1 || seal[0] != 2) throw VerifyError("bad rv32im seal version");
    seal++;
    len--;
  }
  ReadIOP iop(seal, len, suite);
  iop.defer = true;  // openings hashed after the transcript, on several threads (check_pending)
  iop.backend = backend;  // or in one device launch
  // Poseidon254 with its openings on the device: the 31 pair hashes above each tree's top layer
  // (7 trees) stay serial on this thread, as in the host check. R0_VERIFY_P254_TOPS=1 (read at each
  // check, as R0_MERKLE_OPEN_QUAD is) deals them over the opening threads instead (hash_tops):
  // measured and not kept as the default, the thread starts cost more than the hashes (DESIGN.md
  // section 7 item 4).
  if (backend && suite == 2) {
    const char* e = std::getenv("R0_VERIFY_P254_TOPS");
    if (e && std::strtol(e, nullptr, 10) != 0) iop.top_threads = verify_threads();
  }
  uint32_t psi[16], ci[16];
  for (int i = 0; i < 16; i++) {
    psi[i] = fp_encode(uint8_t(PROOF_SYSTEM_INFO[i]));
    ci[i] = fp_encode(uint8_t(c.circuit_info[i]));
  }
  iop.commit(hash_elems(suite, psi, 16));
  iop.commit(hash_elems(suite, ci, 16));
  const uint32_t* header = iop.read_elems(c.output_size + 1);
  iop.commit(hash_elems(suite, header, c.output_size + 1));
  const uint32_t po2 = header[c.output_size];
  if (po2 < 2 || po2 > 24) throw VerifyError("po2 out of range");
  const size_t domain = INV_RATE * (size_t(1) << po2);
  // groups in commit order: code, data, then (after the mix draw) accum (mod.rs:215-244)
  MerkleVerifier code(iop, domain, c.group_sizes[1]);
  // check_code(po2, code_root) (mod.rs:531): e.g. the recursion control-id inclusion check
  // (zkvm/src/receipt/succinct.rs:143-157) is made against the allow-list the caller passes
  if (code_root_out) memcpy(code_root_out, code.root.w, 32);
  if (n_code_roots) {
    bool found = false;
    for (size_t i = 0; i < n_code_roots && !found; i++) found = same(digest_of(code_roots + 8 * i), code.root);
    if (!found) throw VerifyError("code root is not in the allowed set");
  }
  MerkleVerifier data(iop, domain, c.group_sizes[2]);
  std::vector<uint32_t> mix(c.mix_size);
  for (auto& m : mix) m = iop.rng->random_elem();
  MerkleVerifier accum(iop, domain, c.group_sizes[0]);
  const MerkleVerifier* groups[3] = {&accum, &code, &data};
  const TapView taps{c.taps, c.n_taps, c.combo_taps, c.combo_begin, c.combos_count};
  verify_validity_and_fri(iop, taps, po2, groups, check_validity, [&](FpExt poly_mix, const FpExt* eval_u) {
    return poly_ext(c, mix.data(), header, eval_u, poly_mix);
  });
  return po2;
}

}  // namespace
}  // namespace r0

using namespace r0;

static const char* verify_entry(const char* circuit, int suite, const uint32_t* seal, size_t seal_len,
                                bool check_validity, const uint32_t* code_roots, size_t n_code_roots,
                                uint32_t* code_root_out, uint32_t* po2_out, vfy::OpeningBackend backend = nullptr) {
  try {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
    R0_REQUIRE(seal || seal_len == 0, "seal is NULL");
    R0_REQUIRE(code_roots || n_code_roots == 0, "code_roots is NULL");
    uint32_t po2 =
        verify_seal(*c, suite, seal, seal_len, check_validity, code_roots, n_code_roots, code_root_out, backend);
    if (po2_out) *po2_out = po2;
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}

extern "C" const char* r0hip_verify_seal(const char* circuit, int suite, const uint32_t* seal, size_t seal_len,
                                         const uint32_t* h_code_roots, size_t n_code_roots,
                                         uint32_t* h_code_root_out, uint32_t* po2_out) {
  return verify_entry(circuit, suite, seal, seal_len, true, h_code_roots, n_code_roots, h_code_root_out, po2_out);
}

extern "C" const char* r0hip_testing_verify_seal_structure(const char* circuit, int suite, const uint32_t* seal,
                                                           size_t seal_len, uint32_t* po2_out) {
  return verify_entry(circuit, suite, seal, seal_len, false, nullptr, 0, nullptr, po2_out);
}

// where = DEVICE: the host check with the device opening backend. Poseidon254 keeps the host
// openings unless r0hip_set_verify_device_poseidon254 is on, read here. The call drains and hands
// the thread's memory back, as every entry point that gives the host a verdict does (api.cpp
// wrap); nothing here creates a stream on a path that launches nothing.
static const char* verify_entry_on(int where, const char* circuit, int suite, const uint32_t* seal, size_t seal_len,
                                   bool check_validity, const uint32_t* code_roots, size_t n_code_roots,
                                   uint32_t* code_root_out, uint32_t* po2_out) {
  if (where == R0HIP_VERIFY_HOST)
    return verify_entry(circuit, suite, seal, seal_len, check_validity, code_roots, n_code_roots, code_root_out, po2_out);
  if (where != R0HIP_VERIFY_DEVICE)
    return strdup(("r0hip: where = " + std::to_string(where) + " is neither R0HIP_VERIFY_HOST nor R0HIP_VERIFY_DEVICE")
                      .c_str());
  const char* err = verify_entry(circuit, suite, seal, seal_len, check_validity, code_roots, n_code_roots,
                                 code_root_out, po2_out,
                                 suite == 2 && !verify_device_poseidon254() ? nullptr : device_openings);
  drain_after_error();  // a throw may have left work queued; a clean return has drained already
  call_drained();
  release_thread_memory();
  return err;
}

extern "C" const char* r0hip_verify_seal_on(int where, const char* circuit, int suite, const uint32_t* seal,
                                            size_t seal_len, const uint32_t* h_code_roots, size_t n_code_roots,
                                            uint32_t* h_code_root_out, uint32_t* po2_out) {
  return verify_entry_on(where, circuit, suite, seal, seal_len, true, h_code_roots, n_code_roots, h_code_root_out,
                         po2_out);
}

extern "C" const char* r0hip_testing_verify_seal_structure_on(int where, const char* circuit, int suite,
                                                              const uint32_t* seal, size_t seal_len,
                                                              uint32_t* po2_out) {
  return verify_entry_on(where, circuit, suite, seal, seal_len, false, nullptr, 0, nullptr, po2_out);
}

extern "C" const char* r0hip_set_verify_device_poseidon254(int on) {
  if (on != 0 && on != 1)
    return strdup(("r0hip_set_verify_device_poseidon254: on = " + std::to_string(on) + " is neither 0 nor 1").c_str());
  g_verify_device_p254.store(on, std::memory_order_relaxed);
  return nullptr;
}

extern "C" const char* r0hip_constraint_term(const char* circuit, const uint32_t* h_taps, const uint32_t* h_mix,
                                             const uint32_t* h_global, const uint32_t* h_poly_mix, int32_t* term) {
  try {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, "r0hip_constraint_term: " + unknown_circuit(circuit));
    R0_REQUIRE(h_taps, "r0hip_constraint_term: h_taps is NULL");
    R0_REQUIRE(h_mix, "r0hip_constraint_term: h_mix is NULL");
    R0_REQUIRE(h_global, "r0hip_constraint_term: h_global is NULL");
    R0_REQUIRE(h_poly_mix, "r0hip_constraint_term: h_poly_mix is NULL");
    R0_REQUIRE(term, "r0hip_constraint_term: term is NULL");
    *term = constraint_term(*c, h_taps, h_mix, h_global, vfy::load_ext(h_poly_mix));
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}

extern "C" const char* r0hip_poly_ext(const char* circuit, const uint32_t* h_mix, const uint32_t* h_global,
                                      const uint32_t* h_eval_u, const uint32_t* h_poly_mix, uint32_t* h_out) {
  try {
    const CircuitDef* c = find_circuit(circuit ? circuit : "");
    R0_REQUIRE(c, unknown_circuit(circuit));
    R0_REQUIRE(h_mix && h_global && h_eval_u && h_poly_mix && h_out, "poly_ext: null argument");
    std::vector<FpExt> eval_u(c->n_taps);
    for (size_t i = 0; i < c->n_taps; i++) eval_u[i] = vfy::load_ext(h_eval_u + 4 * i);
    FpExt r = poly_ext(*c, h_mix, h_global, eval_u.data(), vfy::load_ext(h_poly_mix));
    memcpy(h_out, r.c, 16);
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}
