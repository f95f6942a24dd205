// Stand-alone check of the run-time circuit validator and bytecode compiler
// (risc0_amd/csrc/circuit_rt.cpp), built by tests/test_circuit_rt_host.py with
// -fsanitize=address,undefined and run as a program of its own.
//   circuit_rt_check good <tables> <max fp slots> <max ext slots>
//       the tables must validate; the compiled program is walked beside the constraint program:
//       every operand must be the leaf it names or a slot that holds exactly the value the
//       record names (so no slot is read before it is written or after it was reused), every
//       slot must be below the counts the slot file is sized by, and the counts within the bounds
//   circuit_rt_check bad <tables>
//       the tables must be refused; the message goes to stdout
// <tables>: a text file of lines "<key> <count> <values...>" (and "name 1 <name>", "info 16 <bytes>").
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "circuit_rt.h"

using namespace r0::rt;

struct Loaded {
  std::string name;
  std::map<std::string, std::vector<int64_t>> v;
  std::vector<uint32_t> u32[8];
  std::vector<int32_t> args;
  r0hip_circuit_tables t{};
};

static const std::vector<uint32_t>& words(Loaded& L, int slot, const char* key) {
  for (int64_t x : L.v[key]) L.u32[slot].push_back(uint32_t(x));
  return L.u32[slot];
}

static void load(const char* path, Loaded& L) {
  std::ifstream in(path);
  if (!in) {
    std::cerr << "cannot read " << path << "\n";
    exit(2);
  }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string key;
    size_t n;
    if (!(ss >> key >> n)) continue;
    if (key == "name") {
      ss >> L.name;
      continue;
    }
    std::vector<int64_t>& v = L.v[key];
    for (size_t i = 0; i < n; i++) {
      int64_t x;
      ss >> x;
      v.push_back(x);
    }
  }
  auto one = [&](const char* k) { return size_t(L.v[k].empty() ? 0 : L.v[k][0]); };
  r0hip_circuit_tables& t = L.t;
  t.name = L.name.c_str();
  t.taps = words(L, 0, "taps").data();
  t.n_taps = one("n_taps");
  t.combo_taps = words(L, 1, "combo_taps").data();
  t.n_combo_taps = L.u32[1].size();
  t.combo_begin = words(L, 2, "combo_begin").data();
  t.combos_count = one("combos_count");
  t.group_begin = words(L, 3, "group_begin").data();
  t.n_groups = one("n_groups");
  t.group_sizes = words(L, 4, "group_sizes").data();
  t.poly_mix_powers = words(L, 5, "poly_mix_powers").data();
  t.n_poly_mix = L.u32[5].size();
  for (size_t i = 0; i < 16 && i < L.v["info"].size(); i++) t.info[i] = uint8_t(L.v["info"][i]);
  t.mix_size = one("mix_size");
  t.output_size = one("output_size");
  for (int64_t x : L.v["eval_args"]) L.args.push_back(int32_t(x));
  t.eval_args = L.args.data();
  t.n_eval_args = L.args.size();
  t.ir = words(L, 6, "ir").data();
  t.n_ir = one("n_ir");
}

#define CHECK(cond, msg)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::cout << "FAILED: " << msg << " (record " << k << ")\n";  \
      return 1;                                                     \
    }                                                               \
  } while (0)

static int walk(const r0hip_circuit_tables& t, const Programs& p, size_t max_fp, size_t max_ext) {
  const std::vector<uint8_t> type = infer_types(t.ir, t.n_ir);
  const int64_t kEmpty = -1;
  std::vector<int64_t> holds[2] = {std::vector<int64_t>(p.n_fp_slots, kEmpty),
                                   std::vector<int64_t>(p.n_ext_slots, kEmpty)};
  size_t pc = 0;
  size_t k = 0;
  // an operand of the bytecode against the id the constraint program names
  auto operand_ok = [&](uint32_t kind, uint32_t value, uint32_t id) -> bool {
    const uint32_t* r = t.ir + 6 * size_t(id);
    switch (r[0]) {
      case IR_C: return kind == K_FP_IMM && value == r[2];
      case IR_E:
        return kind == K_EXT_IMM && size_t(value) * 4 + 4 <= p.consts.size() &&
               std::equal(r + 2, r + 6, p.consts.begin() + size_t(value) * 4);
      case IR_L:
        return kind == K_TAP && value == r[2] && value < p.taps_check.size() && value < p.taps_rows.size() &&
               p.taps_check[value].arg < t.n_eval_args && p.taps_check[value].back == 4 * p.taps_rows[value].back &&
               p.taps_check[value].col < t.group_sizes[t.taps[5 * size_t(value) + 2]];
      case IR_G: {
        const uint32_t arg = value >> 24, idx = value & 0xFFFFFFu;
        return kind == K_WORD && arg < t.n_eval_args && t.eval_args[arg] == (r[2] ? -2 : -1) && idx == r[3] &&
               idx < (r[2] ? t.output_size : t.mix_size);
      }
      default: {
        const uint32_t want = type[id] ? K_EXT_SLOT : K_FP_SLOT;
        return kind == want && value < holds[type[id]].size() && holds[type[id]][value] == int64_t(id);
      }
    }
  };
  for (k = 0; k < t.n_ir; k++) {
    const uint32_t* r = t.ir + 6 * k;
    if (r[0] < IR_ADD) continue;
    CHECK(pc < p.code.size(), "the bytecode ends early");
    const Record& c = p.code[pc++];
    const uint32_t kx = c.kinds & 15, ky = (c.kinds >> 4) & 15, ka = (c.kinds >> 8) & 15;
    if (r[0] == IR_R) {
      CHECK(c.op >> 2 == B_RET, "the r record is not a RET");
      CHECK(operand_ok(kx, c.x, r[1]), "RET reads something other than the result");
      CHECK(bool(c.op & 1) == bool(type[r[1]]), "RET's type bit");
      break;
    }
    if (r[0] == IR_A || r[0] == IR_B) {
      CHECK(c.op >> 2 == (r[0] == IR_A ? B_ACC_A : B_ACC_B), "opcode");
      CHECK(operand_ok(ka, c.acc, r[2]) && kind_is_ext(ka), "the accumulator operand");
      CHECK(operand_ok(kx, c.x, r[3]), "operand x");
      if (r[0] == IR_B) CHECK(operand_ok(ky, c.y, r[4]), "operand y");
      CHECK(c.k == r[r[0] == IR_A ? 4 : 5] && c.k < t.n_poly_mix, "the power index");
      CHECK(bool(c.op & 1) == bool(type[r[3]]), "x's type bit");
      if (r[0] == IR_B) CHECK(bool(c.op & 2) == bool(type[r[4]]), "y's type bit");
    } else {
      CHECK(c.op >> 2 == (r[0] == IR_ADD ? B_ADD : r[0] == IR_SUB ? B_SUB : B_MUL), "opcode");
      CHECK(operand_ok(kx, c.x, r[2]), "operand x");
      CHECK(operand_ok(ky, c.y, r[3]), "operand y");
      CHECK(bool(c.op & 1) == bool(type[r[2]]) && bool(c.op & 2) == bool(type[r[3]]), "the type bits");
    }
    const int ty = type[k];
    CHECK(c.dst < holds[ty].size(), "dst is not below the slot count");
    holds[ty][c.dst] = int64_t(k);
  }
  CHECK(pc == p.code.size(), "records left over");
  std::cout << "records " << p.code.size() << " fp_slots " << p.n_fp_slots << " ext_slots " << p.n_ext_slots
            << " modmuls " << p.modmuls << "\n";
  if (p.n_fp_slots > max_fp || p.n_ext_slots > max_ext) {
    std::cout << "FAILED: slot counts above the bounds " << max_fp << ", " << max_ext << "\n";
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  Loaded L;
  load(argv[2], L);
  const std::string bad = validate(L.t);
  if (mode == "bad") {
    if (bad.empty()) {
      std::cout << "ACCEPTED\n";
      return 1;
    }
    std::cout << bad << "\n";
    return 0;
  }
  if (!bad.empty()) {
    std::cout << "FAILED: refused: " << bad << "\n";
    return 1;
  }
  const Programs p = compile(L.t);
  return walk(L.t, p, argc > 3 ? strtoul(argv[3], nullptr, 10) : ~size_t(0), argc > 4 ? strtoul(argv[4], nullptr, 10) : ~size_t(0));
}
