// Segment prover driving the HIP HAL: the STARK protocol of risc0-zkp
//   risc0/zkp/src/prove/prover.rs:38-393   (make_coeffs, commit_group, finalize)
//   risc0/zkp/src/prove/poly_group.rs:55-83, merkle.rs:54-140, fri.rs:39-126
//   risc0/zkp/src/merkle.rs:39-67, core/poly.rs:23-89
// as driven by the circuit segment provers
//   risc0/circuit/rv32im/src/prove/hal/mod.rs:143-224 (rv32im)
//   risc0/circuit/recursion/src/prove/mod.rs:164-230  (recursion)
//
// Every polynomial, evaluation domain and Merkle tree stays resident in HBM; the
// host only holds the transcript. Kernels are queued on one stream and the host
// synchronises only where the protocol needs a value back: each Merkle root
// (Fiat-Shamir), the out-of-domain evaluations, the division remainders, the
// final FRI coefficients and one batched gather of every query opening.
#include <chrono>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/r0hip.h"
#include "circuit.h"
#include "devmem.h"
#include "ec_zero_scan.h"
#include "eval_interp.h"
#include "plugin.h"
#include "runtime.h"
#include "transcript.h"

namespace r0 {

// launchers implemented in eltwise.hip (declared here to keep runtime.h small)
void combos_sub(hipStream_t s, uint32_t* combos, const uint32_t* deltas, size_t rows, size_t width,
                size_t cycles);
void gather_words(hipStream_t s, uint32_t* dst, const uint32_t* const* bases, const uint32_t* base_id,
                  const uint64_t* offsets, size_t n);

namespace {

constexpr size_t INV_RATE = 4, QUERIES = 50, FRI_FOLD = 16, FRI_MIN_DEGREE = 256, EXT = 4,
                 CHECK_SIZE = INV_RATE * EXT;
const char PROOF_SYSTEM_INFO[] = "RISC0_STARK:v1__";  // adapter.rs:120

size_t log2_exact(size_t v) {
  size_t r = 0;
  while ((size_t(1) << r) < v) r++;
  R0_REQUIRE((size_t(1) << r) == v, "size is not a power of two");
  return r;
}

// host copies through a stream-ordered D2H followed by a sync
void d2h(void* h, const void* d, size_t bytes) { download(h, d, bytes); }
template <typename T>
uint32_t* upload(const std::vector<T>& v, int slot) {
  size_t bytes = v.size() * sizeof(T);
  uint32_t* d = static_cast<uint32_t*>(scratch(bytes ? bytes : 16, slot));
  upload_async(d, v.data(), bytes);
  return d;
}

struct Profile {
  std::vector<std::pair<std::string, hipEvent_t>> marks;
  void mark(const std::string& name) {
    hipEvent_t e;
    HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventRecord(e, stream()));
    marks.push_back({name, e});
  }
  std::string finish() {
    HIP_OK(hipStreamSynchronize(stream()));
    std::ostringstream os;
    for (size_t i = 1; i < marks.size(); i++) {
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, marks[i - 1].second, marks[i].second));
      os << marks[i].first << "=" << ms << ";";
    }
    for (auto& m : marks) (void)hipEventDestroy(m.second);
    marks.clear();
    return os.str();
  }
};

// merkle.rs:39-67 + prove/merkle.rs:26-140
struct MerkleTree {
  size_t rows = 0, cols = 0, layers = 0, top_size = 1;
  const uint32_t* matrix = nullptr;  // device, owned by the PolyGroup / FRI round
  DevBuf nodes;                      // heap of 2*rows digests, root at 1
  Digest root;
  std::vector<uint32_t> top;  // nodes[top_size .. 2*top_size)

  void build(int suite, const uint32_t* m, size_t r, size_t c) {
    DevBuf n(r * 2 * 8);
    {
      Span sp("commit");  // prove/merkle.rs:85
      merkle_tree(stream(), suite, n.p, m, r, c);
    }
    finish(std::move(n), m, r, c);
  }
  // the leaves are already in leaf_nodes[r .. 2r) (hash_rows_range as the matrix arrived)
  void build_from_leaves(int suite, DevBuf leaf_nodes, const uint32_t* m, size_t r, size_t c) {
    {
      Span sp("commit");
      merkle_layers(stream(), suite, leaf_nodes.p, r, c);
    }
    finish(std::move(leaf_nodes), m, r, c);
  }
  static size_t top_size_of(size_t r) {
    const size_t layers = log2_exact(r);
    size_t top_layer = 0;
    for (size_t i = 1; i < layers; i++) {
      if ((size_t(1) << i) > QUERIES) break;
      top_layer = i;
    }
    return size_t(1) << top_layer;
  }
  void finish(DevBuf n, const uint32_t* m, size_t r, size_t c) {
    // root (node 1) .. end of the top layer in one copy
    std::vector<uint32_t> h((2 * top_size_of(r) - 1) * 8);
    d2h(h.data(), n.p + 8, h.size() * 4);
    finish_from(std::move(n), m, r, c, h.data());
  }
  // the same from a host copy `h` of those words (a CachedGroup's): nothing is read back
  void finish_from(DevBuf n, const uint32_t* m, size_t r, size_t c, const uint32_t* h) {
    rows = r;
    cols = c;
    matrix = m;
    nodes = std::move(n);
    layers = log2_exact(rows);
    top_size = top_size_of(rows);
    memcpy(root.w, h, 32);
    top.assign(h + (top_size - 1) * 8, h + (2 * top_size - 1) * 8);
  }
  void commit(WriteIOP& iop) const {
    iop.write(top.data(), top.size());
    iop.commit(root);
  }
};

// From po2 = 12 the coefficient rows stay in the bit-reversed order the inverse NTT leaves
// (the order the forward NTT takes): evaluate_any reads them with bit-reversed power tables
// and mix_poly_coeffs is elementwise, so the only natural-order consumer is combos_divide,
// which gets the (combo_count + 1) mixed rows reversed instead of every trace column.
bool coeffs_stay_bitrev(size_t po2) { return po2 >= kEvalBitrevMinLog; }

struct PolyGroup {
  DevBuf coeffs;
  size_t count = 0;
  bool bitrev = false;  // coeffs rows in bit-reversed order
  DevBuf evaluated;
  MerkleTree tree;
  // poly_group.rs:63-83 (coeffs already interpolated + zk-shifted)
  PolyGroup(int suite, DevBuf c, size_t cnt, size_t po2)
      : coeffs(std::move(c)), count(cnt), bitrev(coeffs_stay_bitrev(po2)) {
    size_t size = size_t(1) << po2, domain = size * INV_RATE;
    evaluated = DevBuf(count * domain);
    ntt_evaluate(stream(), evaluated.p, coeffs.p, count, uint32_t(po2 + 2), 2);
    if (!bitrev) bit_reverse(stream(), coeffs.p, count, uint32_t(po2));
    tree.build(suite, evaluated.p, domain, count);
  }
  // everything already queued (commit_group_device); the tree top is read here
  PolyGroup(GroupWork w, size_t po2)
      : coeffs(std::move(w.coeffs)), count(w.count), bitrev(coeffs_stay_bitrev(po2)), evaluated(std::move(w.evaluated)) {
    tree.finish(std::move(w.nodes), evaluated.p, (size_t(1) << po2) * INV_RATE, count);
  }
  // a group committed earlier and kept (CachedGroup): every buffer is borrowed, so nothing here
  // frees or writes it, and the tree top comes from the host copy
  PolyGroup(const CachedGroup& g, size_t po2) : count(g.count), bitrev(coeffs_stay_bitrev(po2)) {
    const size_t size = size_t(1) << po2, domain = size * INV_RATE;
    coeffs = DevBuf::borrow(g.coeffs, count * size);
    evaluated = DevBuf::borrow(g.evaluated, count * domain);
    tree.finish_from(DevBuf::borrow(g.nodes, domain * 2 * 8), evaluated.p, domain, count, g.top);
  }
  // coefficients (natural order below po2 12), evaluations and leaf digests already made
  // chunk by chunk
  PolyGroup(int suite, DevBuf c, DevBuf ev, DevBuf leaf_nodes, size_t cnt, size_t po2)
      : coeffs(std::move(c)), count(cnt), bitrev(coeffs_stay_bitrev(po2)), evaluated(std::move(ev)) {
    tree.build_from_leaves(suite, std::move(leaf_nodes), evaluated.p, (size_t(1) << po2) * INV_RATE, count);
  }
};

FpExt fe_from_words(const uint32_t* w) { return FpExt{{w[0], w[1], w[2], w[3]}}; }

// core/poly.rs (host, tiny)
FpExt poly_eval(const std::vector<FpExt>& c, FpExt x) {
  FpExt mul = fe_one(), tot = fe_zero();
  for (auto& v : c) {
    tot = fe_add(tot, fe_mul(v, mul));
    mul = fe_mul(mul, x);
  }
  return tot;
}
FpExt poly_divide_host(std::vector<FpExt>& p, FpExt z) {
  FpExt cur = fe_zero();
  for (size_t i = p.size(); i-- > 0;) {
    FpExt next = fe_add(fe_mul(z, cur), p[i]);
    p[i] = cur;
    cur = next;
  }
  return cur;
}
// poly.rs:41-78 (the reference clears the whole tail of `out`; later registers overwrite it)
void poly_interpolate(FpExt* out, size_t out_len, const FpExt* x, const FpExt* fx, size_t size) {
  if (size == 1) {
    out[0] = fx[0];
    return;
  }
  if (size == 2) {
    out[1] = fe_mul(fe_sub(fx[1], fx[0]), fe_inv(fe_sub(x[1], x[0])));
    out[0] = fe_sub(fx[0], fe_mul(out[1], x[0]));
    return;
  }
  std::vector<FpExt> ft(size + 1, fe_zero());
  ft[0] = fe_one();
  for (size_t i = 0; i < size; i++)
    for (size_t j = i + 1; j-- > 0;) {
      FpExt v = ft[j];
      ft[j + 1] = fe_add(ft[j + 1], v);
      ft[j] = fe_mul(ft[j], fe_neg(x[i]));
    }
  for (size_t i = 0; i < out_len; i++) out[i] = fe_zero();
  for (size_t i = 0; i < size; i++) {
    std::vector<FpExt> fr = ft;
    poly_divide_host(fr, x[i]);
    FpExt mul = fe_mul(fx[i], fe_inv(poly_eval(fr, x[i])));
    for (size_t j = 0; j < size; j++) out[j] = fe_add(out[j], fe_mul(mul, fr[j]));
  }
}

std::vector<FpExt> map_pow(FpExt base, const uint32_t* exps, size_t n) {  // field/mod.rs:243-270
  std::vector<FpExt> r;
  if (!n) return r;
  r.push_back(fe_pow(base, exps[0]));
  for (size_t i = 1; i < n; i++)
    r.push_back(exps[i] == exps[i - 1] + 1 ? fe_mul(r.back(), base)
                                           : fe_mul(r.back(), fe_pow(base, exps[i] - exps[i - 1])));
  return r;
}

}  // namespace

namespace {
GroupWork group_buffers(size_t cols, size_t po2) {
  const size_t n = size_t(1) << po2, domain = n * INV_RATE;
  GroupWork w;
  w.count = cols;
  w.coeffs = DevBuf(cols * n);
  w.evaluated = DevBuf(cols * domain);
  w.nodes = DevBuf(domain * 2 * 8);
  return w;
}
void commit_group_queue(hipStream_t s, int suite, uint32_t* coeffs, uint32_t* evaluated, uint32_t* nodes, size_t count,
                        const uint32_t* witness, size_t po2) {
  const size_t domain = (size_t(1) << po2) * INV_RATE;
  ntt_interpolate_from(s, coeffs, witness, count, uint32_t(po2), true);
  ntt_evaluate(s, evaluated, coeffs, count, uint32_t(po2 + 2), 2);
  if (!coeffs_stay_bitrev(po2)) bit_reverse(s, coeffs, count, uint32_t(po2));
  merkle_tree(s, suite, nodes, evaluated, domain, count);
}
void commit_group_queue(hipStream_t s, int suite, GroupWork& w, const uint32_t* witness, size_t po2) {
  commit_group_queue(s, suite, w.coeffs.p, w.evaluated.p, w.nodes.p, w.count, witness, po2);
}
}  // namespace

// commit_group's device half into buffers the caller owns (cols * 2^po2, cols * 2^(po2+2) and
// 16 * 2^(po2+2) words), then the host copy of the tree's root and top layers a CachedGroup
// carries; this thread's stream is drained on return.
std::vector<uint32_t> commit_group_keep(hipStream_t s, int suite, uint32_t* coeffs, uint32_t* evaluated, uint32_t* nodes,
                                        const uint32_t* witness, size_t cols, size_t po2) {
  commit_group_queue(s, suite, coeffs, evaluated, nodes, cols, witness, po2);
  std::vector<uint32_t> h((2 * MerkleTree::top_size_of((size_t(1) << po2) * INV_RATE) - 1) * 8);
  d2h(h.data(), nodes + 8, h.size() * 4);
  return h;
}

// commit_group's device half on stream s: interpolate (zk shift fused), evaluate on the 4x
// domain, row hashes and tree layers, the kernels of commit_group in its order. Nothing is
// read back: PolyGroup(GroupWork, po2) reads the tree top.
GroupWork commit_group_device(hipStream_t s, int suite, const uint32_t* witness, size_t cols, size_t po2) {
  GroupWork w = group_buffers(cols, po2);
  commit_group_queue(s, suite, w, witness, po2);
  return w;
}
// The same on side stream k (r0hip_set_proof_streams >= 2), beside what the caller queues on the
// main stream next. The buffers are taken first and the fork comes after, so the side stream
// runs after every earlier use of those blocks and of `witness` on the main stream. The caller
// joins k before anything reads the group (runtime.h: every function that forks has joined
// before it returns; after a throw in between, drain_after_error waits for the side stream).
GroupWork commit_group_side(int k, int suite, const uint32_t* witness, size_t cols, size_t po2) {
  GroupWork w = group_buffers(cols, po2);
  fork(k);
  commit_group_queue(side_stream(k), suite, w, witness, po2);
  return w;
}

namespace {
// What the generated kernels of either family (evalcheck.h) read besides the result buffer, for
// groups of `domain` rows: the poly_mix powers and folded products with their NBETA multiples,
// the argument and column base pointers, the lane-independent values (from host copies of mix and
// global, read back into hm/hg when the caller has none and the kernels need them) and the
// scratch of the materialised values. `args` backs e.args and outlives the launch.
void ec_tables(const CircuitDef& c, const EvalCheckInfo& info, const uint32_t* const* groups, const uint32_t* mix,
               const uint32_t* global, FpExt poly_mix, size_t domain, const uint32_t*& h_mix, const uint32_t*& h_global,
               std::vector<uint32_t>& hm, std::vector<uint32_t>& hg, std::vector<const uint32_t*>& args,
               EvalCheckArgs& e) {
  std::vector<FpExt> pm = map_pow(poly_mix, c.poly_mix_powers, c.n_poly_mix);
  R0_REQUIRE(pm.size() >= size_t(info.npm), "poly_mix table shorter than the kernels expect");
  pm.resize(info.npm);
  for (int j = 0, k = 0; j < info.ncombos; j++) {
    int n = info.combos[k++];
    FpExt prod = fe_one();
    for (int q = 0; q < n; q++) prod = fe_mul(prod, pm[info.combos[k++]]);
    pm.push_back(prod);
  }
  args.resize(c.n_eval_args);
  for (size_t i = 0; i < c.n_eval_args; i++) {
    int a = c.eval_args[i];
    args[i] = a >= 0 ? groups[a] : (a == -1 ? mix : global);
  }
  e.args = args.data();
  e.nargs = args.size();
  // one base pointer per column the generated program reads (saddr-form tap loads)
  std::vector<const uint32_t*> colptr(info.ncols);
  for (int i = 0; i < info.ncols; i++) colptr[i] = args[info.col_arg[i]] + size_t(info.col_idx[i]) * domain;
  e.colptr = reinterpret_cast<const uint32_t* const*>(upload(colptr, kSlotEcColPtr));
  e.poly_mix = upload(pm, kSlotEcPolyMix);
  std::vector<FpExt> pmn(pm.size());
  for (size_t i = 0; i < pm.size(); i++) pmn[i] = fe_mul_fp(pm[i], kNBeta);
  e.poly_mix_nb = upload(pmn, kSlotEcPolyMixNb);
  // the lane-independent values (functions of mix, global and poly_mix only), from host
  // copies of mix and global (read back here when the caller has none)
  std::vector<uint32_t> uv(4 * size_t(info.n_uniform > 0 ? info.n_uniform : 1), 0);
  if (info.n_uniform > 0) {
    if (!h_mix && c.mix_size) {
      hm.resize(c.mix_size);
      d2h(hm.data(), mix, c.mix_size * 4);
      h_mix = hm.data();
    }
    if (!h_global && c.output_size) {
      hg.resize(c.output_size);
      d2h(hg.data(), global, c.output_size * 4);
      h_global = hg.data();
    }
    std::vector<const uint32_t*> hargs(c.n_eval_args, nullptr);
    for (size_t i = 0; i < c.n_eval_args; i++) {
      if (c.eval_args[i] == -1) hargs[i] = h_mix;
      if (c.eval_args[i] == -2) hargs[i] = h_global;
    }
    info.uniform(hargs.data(), reinterpret_cast<const uint32_t*>(pm.data()), uv.data());
  }
  e.uniform = upload(uv, kSlotEcUniform);
  e.mat_fp = static_cast<uint32_t*>(scratch(size_t(info.mat_fp) * domain * 4 + 16, kSlotEcMatFp));
  e.mat_ext = static_cast<uint32_t*>(scratch(size_t(info.mat_ext) * domain * 16 + 16, kSlotEcMatExt));
  e.domain = uint32_t(domain);
}

// The gates (EvalCheckInfo) whose columns are zero in all `domain` points of the buffers as they
// were handed over: one zero_scan launch over the gate columns, then its 8 bytes back, which
// drains the thread's stream. The whole domain is read, so the answer holds for any caller's
// buffers, not only for low-degree extensions of a trace. R0_EC_SKIP=0 (read on every call)
// turns the scan off: no gate is reported, and every kernel runs.
thread_local int t_ec_launched[2] = {0, 0};

uint64_t ec_dead_gates(const EvalCheckInfo& info, const std::vector<const uint32_t*>& args, size_t domain) {
  const char* skip_env = getenv("R0_EC_SKIP");
  if (info.ngates <= 0 || !info.plan || (skip_env && skip_env[0] == '0' && !skip_env[1])) return 0;
  std::vector<const uint32_t*> cols(info.ngates);
  for (int g = 0; g < info.ngates; g++) {
    const int i = info.gate_col[g];
    cols[g] = args[info.col_arg[i]] + size_t(info.col_idx[i]) * domain;
  }
  return zero_scan_mask(cols, domain);
}

// what the launcher will do with e.dead, for eval_check_launched
void ec_count(const EvalCheckInfo& info, uint64_t dead) {
  t_ec_launched[0] = info.plan ? __builtin_popcountll(info.plan(dead)) : info.kernels;
  t_ec_launched[1] = info.kernels;
}

// A circuit registered at run time has no generated kernels: its constraint program is
// interpreted (eval_interp.hip) over n points, the eval_check form into `check` or the rows form
// into `acc`. The poly_mix table is map_pow(poly_mix, poly_mix_powers) and nothing else. The
// records, tap tables and constants are resident for the life of the process, as the circuit is.
struct InterpRun {
  const rt::Programs& p;
  uint32_t lanes;
};
InterpRun run_interp(const CircuitDef& c, bool rows, const uint32_t* const* groups, const uint32_t* mix,
                     const uint32_t* global, FpExt poly_mix, size_t n, const uint32_t* vinv, uint32_t* check,
                     uint32_t* acc) {
  const rt::Programs& p = *c.interp;
  std::vector<const uint32_t*> args(c.n_eval_args);
  for (size_t i = 0; i < c.n_eval_args; i++) {
    const int a = c.eval_args[i];
    args[i] = a >= 0 ? groups[a] : (a == -1 ? mix : global);
    R0_REQUIRE(args[i] || (a == -1 && !c.mix_size) || (a == -2 && !c.output_size),
               std::string(rows ? "constraint_rows" : "eval_check") + ": argument " + std::to_string(i) + " of circuit " +
                   c.name + " is NULL");
  }
  const uint32_t* image = dev_table(std::string("interp:") + c.name, [&] { return interp_device_image(p); });
  const auto* d_args = reinterpret_cast<const uint32_t* const*>(upload(args, kSlotEcColPtr));
  const uint32_t* d_pow = upload(map_pow(poly_mix, c.poly_mix_powers, c.n_poly_mix), kSlotEcPolyMix);
  const uint32_t lanes = interp_chunk_points(p, n);
  auto* slots = static_cast<uint32_t*>(scratch(size_t(lanes) * p.slot_words() * 4 + 16, kSlotEcInterp));
  eval_interp(stream(), rows, p, image, d_args, d_pow, n, slots, lanes, vinv, check, acc);
  return InterpRun{p, lanes};
}
}  // namespace

uint64_t zero_scan_mask(const std::vector<const uint32_t*>& cols, size_t words) {
  const int n = int(cols.size());
  auto* flags = static_cast<uint32_t*>(scratch(8, kSlotEcGateFlags));
  zero_scan(stream(), reinterpret_cast<const uint32_t* const*>(upload(cols, kSlotEcGatePtr)), n, words, flags);
  uint32_t seen[2];
  d2h(seen, flags, sizeof seen);
  return zero_scan_dead(uint64_t(seen[0]) | (uint64_t(seen[1]) << 32), n);
}

void eval_check_launched(int out[2]) noexcept {
  out[0] = t_ec_launched[0];
  out[1] = t_ec_launched[1];
}

// eval_check for one circuit (rv32im/src/prove/hal/cpu.rs:145-207 semantics)
void run_eval_check(const CircuitDef& c, uint32_t* check, const uint32_t* const* groups, const uint32_t* mix,
                    const uint32_t* global, FpExt poly_mix, size_t po2, const uint32_t* h_mix,
                    const uint32_t* h_global) {
  hipStream_t s = stream();
  size_t steps = size_t(1) << po2, domain = steps * INV_RATE;
  // inv((3 * w_D^c)^N - 1) depends only on c mod 4 (w_D^(cN) = w_4^c)
  std::vector<uint32_t> vinv(4);
  uint32_t w = fp_encode(kRouFwd[po2 + 2]);
  for (uint32_t q = 0; q < 4; q++) {
    uint32_t x = fp_pow(w, q);
    uint32_t y = fp_pow(fp_mul(fp_encode(3), x), steps);
    vinv[q] = fp_inv(fp_sub(y, kOne));
  }
  if (c.interp) {  // registered at run time: the interpreter, same algorithmic bytes
    double bytes = 16.0 * domain;
    for (int g = 0; g < 3; g++) bytes += 4.0 * domain * c.group_sizes[g];
    Span span("eval_check");
    KScope ks("eval_check_interp", bytes, double(domain) * (c.interp->modmuls + 4));
    run_interp(c, false, groups, mix, global, poly_mix, domain, upload(vinv, kSlotEcVinv), check, nullptr);
    t_ec_launched[0] = t_ec_launched[1] = 0;
    return;
  }
  EvalCheckInfo info;
  c.info(&info);
  std::vector<uint32_t> hm, hg;
  std::vector<const uint32_t*> args;
  EvalCheckArgs e;
  ec_tables(c, info, groups, mix, global, poly_mix, domain, h_mix, h_global, hm, hg, args, e);
  e.vinv = upload(vinv, kSlotEcVinv);
  e.acc = static_cast<uint32_t*>(scratch(domain * 16, kSlotEcAcc));
  e.check = check;
  {
    static const uint32_t tile_env = [] {
      const char* t = getenv("R0_EC_TILE");
      return t ? uint32_t(strtoul(t, nullptr, 0)) : 0u;
    }();
    e.tile = tile_env;
    // R0_EC_WIDE (experiments, tests): mask of the kernels that take the column-base tap form,
    // read on every call
    const char* wide_env = getenv("R0_EC_WIDE");
    e.wide = wide_env ? int64_t(strtoull(wide_env, nullptr, 0)) : int64_t(-1);
  }
  double bytes = 16.0 * domain;
  for (int g = 0; g < 3; g++) bytes += 4.0 * domain * c.group_sizes[g];
  Span span("eval_check");
  KScope ks("eval_check", bytes, double(domain) * info.modmuls_per_point);
  e.dead = ec_dead_gates(info, args, domain);
  ec_count(info, e.dead);
  c.eval_check(s, e);
}

// The constraint polynomial on the trace rows (runtime.h): eval_check's tables for N rows in
// place of the 4N domain, the groups as they are, no vanishing-polynomial factor. Then the report
// kernel, its 19 words back, and for a bad witness the first bad row's taps and its term.
void constraint_rows_run(const CircuitDef& c, size_t po2, const uint32_t* const* groups, const uint32_t* mix,
                         const uint32_t* global, const uint32_t* h_mix, const uint32_t* h_global, FpExt poly_mix,
                         uint32_t* vals, r0hip_constraint_report* report) {
  hipStream_t s = stream();
  const size_t rows = size_t(1) << po2;
  std::vector<uint32_t> hm, hg;
  std::vector<const uint32_t*> args;
  EvalCheckArgs e;
  e.acc = vals ? vals : static_cast<uint32_t*>(scratch(rows * 16, kSlotEcAcc));
  auto* d_rep = static_cast<uint32_t*>(scratch(19 * 4, kSlotRowsReport));
  if (c.interp) {  // registered at run time: the interpreter, then the same report kernel
    double bytes = 16.0 * rows;
    for (int g = 0; g < 3; g++) bytes += 4.0 * rows * c.group_sizes[g];
    Span span("constraint_rows");
    KScope ks("constraint_rows_interp", bytes, double(rows) * c.interp->modmuls);
    run_interp(c, true, groups, mix, global, poly_mix, rows, nullptr, nullptr, e.acc);
    t_ec_launched[0] = t_ec_launched[1] = 0;
    rows_report(s, e.acc, rows, d_rep);
  } else {
    EvalCheckInfo info;
    c.rows_info(&info);
    ec_tables(c, info, groups, mix, global, poly_mix, rows, h_mix, h_global, hm, hg, args, e);
    e.check = nullptr;
    e.vinv = nullptr;
    e.wide = 0;
    double bytes = 16.0 * rows;
    for (int g = 0; g < 3; g++) bytes += 4.0 * rows * c.group_sizes[g];
    Span span("constraint_rows");
    KScope ks("constraint_rows", bytes, double(rows) * info.modmuls_per_point);
    e.dead = ec_dead_gates(info, args, rows);
    ec_count(info, e.dead);
    c.constraint_rows(s, e);
    rows_report(s, e.acc, rows, d_rep);
  }
  uint32_t rep[19];
  d2h(rep, d_rep, sizeof rep);
  *report = r0hip_constraint_report{};
  report->bad_rows = uint64_t(rep[0]) | (uint64_t(rep[1]) << 32);
  report->first_row = rep[2];
  report->first_term = -1;
  for (int k = 0; k < 16; k++) {
    report->rows[k] = rep[3 + k];
    if (rep[3 + k] != 0xFFFFFFFFu) report->n_rows = uint32_t(k + 1);
  }
  if (!report->bad_rows) return;
  // the first bad row's taps, in tap order, and the term they violate
  std::vector<const uint32_t*> bases(groups, groups + 3);
  std::vector<uint32_t> ids(c.n_taps);
  std::vector<uint64_t> offs(c.n_taps);
  for (size_t t = 0; t < c.n_taps; t++) {
    ids[t] = c.tap(t).group;
    offs[t] = uint64_t(c.tap(t).offset) * rows + ((report->first_row - c.tap(t).back) & uint32_t(rows - 1));
  }
  auto* d_taps = static_cast<uint32_t*>(scratch(c.n_taps * 4, kSlotRowsTaps));
  gather_words(s, d_taps, reinterpret_cast<const uint32_t* const*>(upload(bases, kSlotRowsBases)),
               upload(ids, kSlotRowsIds), reinterpret_cast<const uint64_t*>(upload(offs, kSlotRowsOffs)), c.n_taps);
  std::vector<uint32_t> taps(c.n_taps);
  d2h(taps.data(), d_taps, c.n_taps * 4);
  if (!h_mix && c.mix_size) {
    hm.resize(c.mix_size);
    d2h(hm.data(), mix, c.mix_size * 4);
    h_mix = hm.data();
  }
  if (!h_global && c.output_size) {
    hg.resize(c.output_size);
    d2h(hg.data(), global, c.output_size * 4);
    h_global = hg.data();
  }
  report->first_term = constraint_term(c, taps.data(), h_mix, h_global, poly_mix);
}

namespace {
thread_local bool t_witness_check = false;

// four field words from the OS for a check that must not touch the transcript
FpExt os_random_ext() {
  uint32_t w[8];
  os_random_key(w);
  return FpExt{{w[0] % kP, w[1] % kP, w[2] % kP, w[3] % kP}};
}
}  // namespace

bool witness_check_mode() noexcept { return t_witness_check; }
bool set_witness_check_mode(bool on) noexcept {
  const bool was = t_witness_check;
  t_witness_check = on;
  return was;
}
FpExt constraint_rows_poly_mix(const uint32_t* h_poly_mix) {
  return h_poly_mix ? fe_from_words(h_poly_mix) : os_random_ext();
}

namespace {

struct Prover {
  const CircuitDef& c;
  int suite;
  WriteIOP iop;
  size_t po2 = 0, cycles = 0;
  std::unique_ptr<PolyGroup> groups[3];
  Profile* prof;

  Prover(const CircuitDef& circ, int s, Profile* p) : c(circ), suite(s), iop(s), prof(p) {}

  // prover.rs:38-48 + 81-108; zk_shift fused into the interpolation's last pass
  // A group still uploading in column chunks (the segment pipeline): each chunk's
  // interpolate, evaluate, bit-reverse and leaf-hash range run as soon as it lands, so the
  // group's NTTs and row hashes overlap its own upload. Same words as commit_group.
  void commit_group_streamed(size_t g, int up_group, const uint32_t* witness, const UploadGate& up) {
    Span span("commit_group");
    hipStream_t s = stream();
    const size_t gs = c.group_size(g), n = cycles, domain = n * INV_RATE, ch = up.chunk_cols(up_group);
    DevBuf coeffs(gs * n), evaluated(gs * domain), nodes(domain * 2 * 8), state(domain * 8);
    for (size_t c0 = 0; c0 < gs; c0 += ch) {
      const size_t cc = std::min(ch, gs - c0);
      up.wait(up_group, c0 + cc, s);
      {
        Span sp("make_coeffs");
        ntt_interpolate_from(s, coeffs.p + c0 * n, witness + c0 * n, cc, uint32_t(po2), true);
      }
      ntt_evaluate(s, evaluated.p + c0 * domain, coeffs.p + c0 * n, cc, uint32_t(po2 + 2), 2);
      if (!coeffs_stay_bitrev(po2)) bit_reverse(s, coeffs.p + c0 * n, cc, uint32_t(po2));
      hash_rows_range(s, suite, nodes.p + domain * 8, state.p, evaluated.p + c0 * domain, domain, cc, c0 == 0,
                      c0 + cc == gs);
    }
    groups[g].reset(new PolyGroup(suite, std::move(coeffs), std::move(evaluated), std::move(nodes), gs, po2));
    groups[g]->tree.commit(iop);
  }

  void commit_group(size_t g, const uint32_t* witness) {
    Span span("commit_group");
    size_t gs = c.group_size(g);
    DevBuf coeffs(gs * cycles);
    {
      Span sp("make_coeffs");
      ntt_interpolate_from(stream(), coeffs.p, witness, gs, uint32_t(po2), true);
    }
    groups[g].reset(new PolyGroup(suite, std::move(coeffs), gs, po2));
    groups[g]->tree.commit(iop);
  }
  // commit_group's transcript half for a group whose device half is queued and joined: the
  // tree top is read, then written and hashed into the transcript
  void commit_group_finish(size_t g, GroupWork w) {
    Span span("commit_group");
    groups[g].reset(new PolyGroup(std::move(w), po2));
    groups[g]->tree.commit(iop);
  }
  // commit_group for a group committed before this proof: no device work, the root enters the
  // transcript where tree.commit puts it
  void commit_group_cached(size_t g, const CachedGroup& cg) {
    Span span("commit_group");
    R0_REQUIRE(cg.count == c.group_size(g), "cached group has another column count");
    groups[g].reset(new PolyGroup(cg, po2));
    groups[g]->tree.commit(iop);
  }

  // prover.rs:111-393
  void finalize(const uint32_t* mix, const uint32_t* global, const uint32_t* h_mix, const uint32_t* h_global) {
    Span span("finalize");
    hipStream_t s = stream();
    FpExt poly_mix = iop.rng->random_ext_elem();
    size_t domain = cycles * INV_RATE;
    DevBuf check(EXT * domain);
    const uint32_t* gptr[3] = {groups[0]->evaluated.p, groups[1]->evaluated.p, groups[2]->evaluated.p};
    run_eval_check(c, check.p, gptr, mix, global, poly_mix, po2, h_mix, h_global);
    if (prof) prof->mark("eval_check");
    ntt_interpolate(s, check.p, EXT, uint32_t(po2 + 2), false);
    PolyGroup check_group(suite, std::move(check), CHECK_SIZE, po2);
    check_group.tree.commit(iop);
    if (prof) prof->mark("check_group");

    FpExt z = iop.rng->random_ext_elem();
    FpExt back_one = fe_from_fp(fp_encode(kRouRev[po2]));
    std::vector<FpExt> all_xs, eval_u;
    Span span_u("eval_u");
    {
      // one batched launch per group; a single host sync for all of them
      std::vector<std::vector<uint32_t>> whichs(3);
      std::vector<std::vector<FpExt>> xss(3);
      size_t total = 0;
      for (size_t id = 0; id < 3; id++) {
        for (size_t t = c.group_begin[id]; t < c.group_begin[id + 1]; t++) {
          whichs[id].push_back(c.tap(t).offset);
          FpExt x = fe_mul(fe_pow(back_one, c.tap(t).back), z);
          xss[id].push_back(x);
          all_xs.push_back(x);
        }
        total += whichs[id].size();
      }
      DevBuf out((total + CHECK_SIZE) * 4);
      size_t off = 0;
      for (size_t id = 0; id < 3; id++) {
        uint32_t* dx = upload(xss[id], kSlotTapXs + int(id));
        batch_evaluate_any_host(s, groups[id]->coeffs.p, groups[id]->count, uint32_t(po2), whichs[id], dx,
                                out.p + off * 4, groups[id]->bitrev);
        off += whichs[id].size();
      }
      std::vector<uint32_t> h(total * 4);
      d2h(h.data(), out.p, h.size() * 4);
      for (size_t i = 0; i < total; i++) eval_u.push_back(fe_from_words(&h[4 * i]));
    }
    std::vector<FpExt> coeff_u(eval_u.size(), fe_zero());
    {
      size_t pos = 0;
      c.regs(0, c.n_taps, [&](size_t cur) {
        size_t sz = c.tap(cur).skip;
        poly_interpolate(&coeff_u[pos], coeff_u.size() - pos, &all_xs[pos], &eval_u[pos], sz);
        pos += sz;
      });
    }
    FpExt z_pow = fe_pow(z, EXT);
    {
      std::vector<uint32_t> which(CHECK_SIZE);
      for (size_t i = 0; i < CHECK_SIZE; i++) which[i] = uint32_t(i);
      std::vector<FpExt> xs(CHECK_SIZE, z_pow);
      DevBuf out(CHECK_SIZE * 4);
      batch_evaluate_any_host(s, check_group.coeffs.p, CHECK_SIZE, uint32_t(po2), which, upload(xs, kSlotCheckXs), out.p,
                              check_group.bitrev);
      std::vector<uint32_t> h(CHECK_SIZE * 4);
      d2h(h.data(), out.p, h.size() * 4);
      for (size_t i = 0; i < CHECK_SIZE; i++) coeff_u.push_back(fe_from_words(&h[4 * i]));
      iop.write(&coeff_u[0].c[0], coeff_u.size() * 4);
      iop.commit(hash_elems(suite, &coeff_u[0].c[0], coeff_u.size() * 4));
    }
    if (prof) prof->mark("eval_u");
    FpExt mix_fri = iop.rng->random_ext_elem();
    Span span_mix("mix_poly_coeffs");

    size_t combo_count = c.combos_count;
    DevBuf combos(cycles * (combo_count + 1) * 4);
    HIP_OK(hipMemsetAsync(combos.p, 0, combos.words * 4, s));
    {
      FpExt cur_mix = fe_one();
      for (size_t id = 0; id < 3; id++) {
        size_t gs = c.group_size(id);
        std::vector<uint32_t> which;
        c.regs(c.group_begin[id], c.group_begin[id + 1], [&](size_t cur) { which.push_back(c.tap(cur).combo); });
        R0_REQUIRE(which.size() == gs, "group registers != group size");
        mix_poly_coeffs(s, combos.p, groups[id]->coeffs.p, upload(which, kSlotMixWhich), which, cur_mix, mix_fri, gs, cycles);
        cur_mix = fe_mul(cur_mix, fe_pow(mix_fri, gs));
      }
      std::vector<uint32_t> which(CHECK_SIZE, uint32_t(combo_count));
      mix_poly_coeffs(s, combos.p, check_group.coeffs.p, upload(which, kSlotMixWhichCheck), which, cur_mix, mix_fri, CHECK_SIZE,
                      cycles);
      R0_REQUIRE(check_group.bitrev == groups[0]->bitrev && groups[1]->bitrev == groups[0]->bitrev &&
                     groups[2]->bitrev == groups[0]->bitrev,
                 "coefficient groups in mixed orders");
      if (check_group.bitrev) bit_reverse_ext(s, combos.p, combo_count + 1, uint32_t(po2));
    }
    if (prof) prof->mark("mix");
    {
      Span sp("divide");
      // combos_prepare (hal/mod.rs:202-234) as per-row deltas on the low coefficients
      size_t width = 1;
      c.regs(0, c.n_taps, [&](size_t cur) { width = std::max<size_t>(width, c.tap(cur).skip); });
      std::vector<FpExt> deltas((combo_count + 1) * width, fe_zero());
      size_t cur_pos = 0;
      FpExt cur = fe_one();
      c.regs(0, c.n_taps, [&](size_t t) {
        size_t sz = c.tap(t).skip, id = c.tap(t).combo;
        for (size_t i = 0; i < sz; i++)
          deltas[id * width + i] = fe_add(deltas[id * width + i], fe_mul(cur, coeff_u[cur_pos + i]));
        cur = fe_mul(cur, mix_fri);
        cur_pos += sz;
      });
      for (size_t i = 0; i < CHECK_SIZE; i++) {
        deltas[combo_count * width] = fe_add(deltas[combo_count * width], fe_mul(cur, coeff_u[cur_pos]));
        cur_pos++;
        cur = fe_mul(cur, mix_fri);
      }
      combos_sub(s, combos.p, upload(deltas, kSlotCombosDeltas), combo_count + 1, width, cycles);
      // combos_divide (hal/mod.rs:236-257; cuda.rs:1034-1048)
      std::vector<std::vector<FpExt>> zs(combo_count + 1);
      for (size_t i = 0; i < combo_count; i++)
        for (uint32_t k = c.combo_begin[i]; k < c.combo_begin[i + 1]; k++)
          zs[i].push_back(fe_mul(z, fe_pow(back_one, c.combo_taps[k])));
      zs[combo_count].push_back(z_pow);
      size_t maxz = 0;
      for (auto& v : zs) maxz = std::max(maxz, v.size());
      DevBuf rem((combo_count + 1) * maxz * 4);
      HIP_OK(hipMemsetAsync(rem.p, 0, rem.words * 4, s));
      poly_divide_rows(s, combos.p, cycles, zs, rem.p);
      std::vector<uint32_t> h(rem.words);
      d2h(h.data(), rem.p, h.size() * 4);
      for (size_t i = 0; i < h.size(); i++)
        R0_REQUIRE(h[i] == 0, "combos_divide: nonzero remainder in chunk " + std::to_string(i / (4 * maxz)));
    }
    if (prof) prof->mark("divide");
    DevBuf final_poly(cycles * EXT);
    Span span_sum("sum");
    eltwise_sum_extelem(s, final_poly.p, combos.p, cycles, combo_count + 1);
    bit_reverse(s, final_poly.p, EXT, uint32_t(po2));
    combos = DevBuf();
    fri_prove(std::move(final_poly), check_group);
  }

  struct Round {
    size_t domain;
    DevBuf evaluated;
    MerkleTree tree;
  };

  // fri.rs:86-126 with all query openings gathered in one device pass
  void fri_prove(DevBuf coeffs, const PolyGroup& check_group) {
    Span span("fri_prove");
    hipStream_t s = stream();
    size_t size = coeffs.words / EXT;
    size_t orig_domain = size * INV_RATE;
    std::vector<std::unique_ptr<Round>> rounds;
    while (size > FRI_MIN_DEGREE) {
      std::unique_ptr<Round> r(new Round);
      r->domain = size * INV_RATE;
      r->evaluated = DevBuf(r->domain * EXT);
      ntt_evaluate(s, r->evaluated.p, coeffs.p, EXT, uint32_t(log2_exact(r->domain)), 2);
      r->tree.build(suite, r->evaluated.p, r->domain / FRI_FOLD, FRI_FOLD * EXT);
      r->tree.commit(iop);
      FpExt fold_mix = iop.rng->random_ext_elem();
      DevBuf out(size / FRI_FOLD * EXT);
      fri_fold(s, out.p, coeffs.p, fold_mix, size / FRI_FOLD);
      coeffs = std::move(out);
      size /= FRI_FOLD;
      rounds.push_back(std::move(r));
    }
    if (prof) prof->mark("fri_fold");
    {
      DevBuf fin(coeffs.words);
      HIP_OK(hipMemcpyAsync(fin.p, coeffs.p, coeffs.words * 4, hipMemcpyDeviceToDevice, s));
      bit_reverse(s, fin.p, EXT, uint32_t(log2_exact(size)));
      std::vector<uint32_t> h(fin.words);
      d2h(h.data(), fin.p, h.size() * 4);
      iop.write(h.data(), h.size());
      iop.commit(hash_elems(suite, h.data(), h.size()));
    }
    // The query loop only writes to the proof, so the positions can all be drawn first.
    std::vector<size_t> positions(QUERIES);
    for (auto& p : positions) p = iop.rng->random_bits(log2_exact(orig_domain));
    std::vector<const uint32_t*> bases;
    std::vector<uint32_t> base_id;
    std::vector<uint64_t> offs;
    auto add_base = [&](const uint32_t* p) {
      bases.push_back(p);
      return uint32_t(bases.size() - 1);
    };
    struct T {
      const MerkleTree* t;
      uint32_t mat, nodes;
    };
    std::vector<T> trees;
    for (auto& g : groups) trees.push_back({&g->tree, add_base(g->tree.matrix), add_base(g->tree.nodes.p)});
    trees.push_back({&check_group.tree, add_base(check_group.tree.matrix), add_base(check_group.tree.nodes.p)});
    std::vector<T> rtrees;
    for (auto& r : rounds) rtrees.push_back({&r->tree, add_base(r->tree.matrix), add_base(r->tree.nodes.p)});
    auto prove = [&](const T& t, size_t idx) {  // prove/merkle.rs:108-140
      const MerkleTree& m = *t.t;
      for (size_t i = 0; i < m.cols; i++) {
        base_id.push_back(t.mat);
        offs.push_back(idx + i * m.rows);
      }
      idx += m.rows;
      while (idx >= 2 * m.top_size) {
        size_t low = idx % 2;
        idx /= 2;
        size_t other = 2 * idx + (1 - low);
        for (size_t k = 0; k < 8; k++) {
          base_id.push_back(t.nodes);
          offs.push_back(other * 8 + k);
        }
      }
    };
    for (size_t pos : positions) {
      for (auto& t : trees) prove(t, pos);
      for (size_t ri = 0; ri < rounds.size(); ri++) {
        size_t group = pos % (rounds[ri]->domain / FRI_FOLD);
        prove(rtrees[ri], group);
        pos = group;
      }
    }
    DevBuf words(offs.size());
    const uint32_t* const* dbases = reinterpret_cast<const uint32_t* const*>(upload(bases, kSlotQueryBases));
    gather_words(s, words.p, dbases, upload(base_id, kSlotQueryIds), reinterpret_cast<const uint64_t*>(upload(offs, kSlotQueryOffs)),
                 offs.size());
    std::vector<uint32_t> h(offs.size());
    d2h(h.data(), words.p, h.size() * 4);
    iop.write(h.data(), h.size());
    if (prof) prof->mark("queries");
  }
};

thread_local std::string g_last_profile;  // per host thread (segments in flight)

}  // namespace

std::string last_profile() { return g_last_profile; }

// circuit/rv32im/src/prove/hal/mod.rs:181-224 (recursion: prove/mod.rs:176-226, no version word)
// `uploads` (optional): the groups may still be uploading; each is waited for just before
// its first use, so a segment's early phases overlap the upload of its later groups
// `cb` (prove_segment_cb): the accum group comes from the caller's function, after the mix
static std::vector<uint32_t> prove_segment_impl(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                                const uint32_t* data, const uint32_t* accum, uint32_t* global,
                                                bool write_version, uint32_t version, std::vector<uint32_t>* mix_out,
                                                const UploadGate* uploads, const AccumStep* acc, GroupWork* code_early,
                                                const CachedGroup* code_cached, const AccumCallback* cb) {
  R0_REQUIRE(suite >= 0 && suite <= 2, "unknown hash suite");
  R0_REQUIRE(!cb || (cb->fn && !accum && !acc), "prove_segment: an accum callback beside an accum group or step");
  R0_REQUIRE(!code_cached || (!code_early && !uploads), "prove_segment: a cached code group with one in flight");
  R0_REQUIRE(!acc || (acc->accum && !accum), "prove_segment: give the accum group or an accumulation, not both");
  R0_REQUIRE(po2 >= 2 && po2 <= 24, "po2 out of range");
  Span span("prove_core");
  hipStream_t s = stream();
  auto gate = [&](int g) {
    if (uploads) uploads->wait(g, SIZE_MAX, s);
  };
  stage_reset();
  Profile prof;
  prof.mark("start");
  Prover p(c, suite, &prof);
  if (write_version) p.iop.proof.push_back(version);
  uint32_t psi[16], ci[16];
  for (int i = 0; i < 16; i++) {
    psi[i] = fp_encode(uint8_t(PROOF_SYSTEM_INFO[i]));
    ci[i] = fp_encode(uint8_t(c.circuit_info[i]));
  }
  p.iop.commit(hash_elems(suite, psi, 16));
  p.iop.commit(hash_elems(suite, ci, 16));
  // header = globals (INVALID -> 0, in place) || po2 as a raw word
  gate(3);
  eltwise_zeroize(s, global, c.output_size);
  std::vector<uint32_t> header(c.output_size + 1);
  d2h(header.data(), global, c.output_size * 4);
  header[c.output_size] = po2;
  p.iop.commit(hash_elems(suite, header.data(), header.size()));
  p.iop.write(header.data(), header.size());
  p.po2 = po2;
  p.cycles = size_t(1) << po2;
  // reference group index, pipeline buffer index (0 code, 1 data, 2 accum)
  auto commit = [&](size_t g, int up_group, const uint32_t* w) {
    const size_t gs = c.group_size(g);
    if (uploads && suite != 2 && gs > uploads->chunk_cols(up_group) && uploads->chunk_cols(up_group) % 16 == 0) {
      p.commit_group_streamed(g, up_group, w, *uploads);
    } else {
      gate(up_group);
      p.commit_group(g, w);
    }
  };
  // r0hip_set_proof_streams >= 2 (never with a group still uploading): the code group's device
  // work runs on side stream 1, started by the caller before its witness generation
  // (code_early) or here, beside the data group's on the main stream. The roots are read and
  // hashed into the transcript in the reference's order, code then data, and the side stream is
  // joined before anything reads the code group's buffers.
  // code_cached (a recursion program handle): the code group was committed when the handle was
  // made; there is no code commit to queue or to fork, whatever r0hip_set_proof_streams says,
  // and the data group is committed as at n = 1.
  if (code_cached) {
    p.commit_group_cached(1, *code_cached);
    prof.mark("commit_code");
    commit(2, 1, data);
    prof.mark("commit_data");
  } else if (code_early || (!uploads && active_proof_streams() >= 2)) {
    GroupWork cw = code_early ? std::move(*code_early) : commit_group_side(1, suite, code, c.group_size(1), po2);
    GroupWork dw = commit_group_device(s, suite, data, c.group_size(2), po2);
    join(1);
    p.commit_group_finish(1, std::move(cw));
    prof.mark("commit_code");
    p.commit_group_finish(2, std::move(dw));
    prof.mark("commit_data");
  } else {
    commit(1, 0, code);
    prof.mark("commit_code");
    commit(2, 1, data);
    prof.mark("commit_data");
  }
  std::vector<uint32_t> mix(c.mix_size);
  for (auto& m : mix) m = p.iop.rng->random_elem();
  if (mix_out) *mix_out = mix;
  DevBuf dmix(mix.size() ? mix.size() : 1);
  upload_async(dmix.p, mix.data(), mix.size() * 4);
  // r0hip_set_witness_check: the three groups are in their final form (the data commit
  // interpolated out of place, the accumulation only read the data): the constraint polynomial on
  // their rows, with a poly_mix of the OS's, so the transcript and the seal are those of the mode
  // off. A violated row ends the proof here, before the accum commit and the 4N work.
  DevBuf cb_accum;  // the callback's accum group: alive until the final drain
  auto check_witness = [&](const uint32_t* accum_group) {
    if (!witness_check_mode()) return;
    gate(0);
    gate(1);
    const uint32_t* wg[3] = {accum_group, code, data};
    r0hip_constraint_report rep;
    constraint_rows_run(c, po2, wg, dmix.p, global, mix.data(), header.data(), constraint_rows_poly_mix(nullptr),
                        nullptr, &rep);
    prof.mark("check_witness");
    if (rep.bad_rows) {
      (void)prof.finish();  // an expected outcome: the marks' events are released
      throw std::runtime_error("constraint check failed: " + std::to_string(rep.bad_rows) + " of " +
                               std::to_string(p.cycles) + " rows, first at cycle " + std::to_string(rep.first_row) +
                               " (term " + std::to_string(rep.first_term) + ")");
    }
  };
  if (acc) {
    Span acc_span("accumulate");
    const size_t rows = p.cycles, cols = c.group_size(0);
    const std::string name = c.name;
    if (acc->fill_invalid) HIP_OK(hipMemsetD32Async(acc->accum, 0xFFFFFFFFu, rows * cols, s));
    if (name == "rv32im") {
      // witgen/mod.rs:182-205: the BigInt states with the final mix, then the step
      rv32im_bigint_inject(s, acc->accum, rows, mix.data(), acc->bigint, acc->n_bigint);
      rv32im_accum(s, data, acc->accum, global, dmix.p, rows, cols, acc->work_cycles);
    } else if (name == "recursion") {
      R0_REQUIRE(acc->n_bigint == 0, "prove_segment: BigInt backs are an rv32im trace record");
      recursion_accum(s, code, global, data, dmix.p, acc->accum, acc->work_cycles, rows);
    } else {
      R0_REQUIRE(false, "prove_segment: no device accumulation for circuit " + name);
    }
    if (!acc->zeroed) eltwise_zeroize(s, acc->accum, rows * cols);
    prof.mark("accumulate");
    check_witness(acc->accum);
    p.commit_group(0, acc->accum);  // nothing to wait for: the group never uploads
  } else if (cb) {
    // r0hip_prove_segment_cb: the group is the prover's, filled by the caller's function once
    // the mix is known. The stream is drained first, so the function sees code and data
    // committed and may write the group by any means; what it queues on `s` is ordered before
    // the zeroize. A message ends the proof here, as a failed witness check does.
    Span acc_span("accumulate");
    const size_t rows = p.cycles, cols = c.group_size(0);
    cb_accum = DevBuf(rows * cols);
    HIP_OK(hipMemsetD32Async(cb_accum.p, 0xFFFFFFFFu, rows * cols, s));
    HIP_OK(hipStreamSynchronize(s));
    const char* msg = cb->fn(cb->user, mix.data(), cb_accum.p, s);
    if (msg) {
      const std::string m = msg;
      (void)prof.finish();
      throw std::runtime_error("accum callback: " + m);
    }
    eltwise_zeroize(s, cb_accum.p, rows * cols);
    prof.mark("accumulate");
    check_witness(cb_accum.p);
    p.commit_group(0, cb_accum.p);
  } else {
    if (witness_check_mode()) {
      gate(2);
      check_witness(accum);
    }
    commit(0, 2, accum);
  }
  prof.mark("commit_accum");
  p.finalize(dmix.p, global, mix.data(), header.data());
  HIP_OK(hipStreamSynchronize(s));
  g_last_profile = prof.finish();
  return std::move(p.iop.proof);
}

std::vector<uint32_t> prove_segment(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                    const uint32_t* data, const uint32_t* accum, uint32_t* global,
                                    bool write_version, uint32_t version, std::vector<uint32_t>* mix_out,
                                    const UploadGate* uploads, const AccumStep* acc, GroupWork* code_early,
                                    const CachedGroup* code_cached) {
  return prove_segment_impl(c, suite, po2, code, data, accum, global, write_version, version, mix_out, uploads, acc,
                            code_early, code_cached, nullptr);
}

std::vector<uint32_t> prove_segment_cb(const CircuitDef& c, int suite, uint32_t po2, const uint32_t* code,
                                       const uint32_t* data, uint32_t* global, bool write_version, uint32_t version,
                                       std::vector<uint32_t>* mix_out, const AccumCallback& cb) {
  return prove_segment_impl(c, suite, po2, code, data, nullptr, global, write_version, version, mix_out, nullptr,
                            nullptr, nullptr, nullptr, &cb);
}

}  // namespace r0
