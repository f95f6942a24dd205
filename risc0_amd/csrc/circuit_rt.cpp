// Circuits registered at run time: the validator and the bytecode compiler (circuit_rt.h).
// Host code only, no HIP header: it runs once per r0hip_circuit_register.
#include "circuit_rt.h"

#include <algorithm>
#include <tuple>

namespace r0 {
namespace rt {
namespace {

constexpr uint32_t kPrime = 0x78000001u;  // bb31.h kP (that header pulls in HIP under hipcc)

struct Tap {
  uint32_t offset, back, group, combo, skip;
};

std::string str(size_t v) { return std::to_string(v); }

// number of id operands of a record (after op, dst)
int n_id_operands(uint32_t op) {
  switch (op) {
    case IR_ADD: case IR_SUB: case IR_MUL: case IR_A: return 2;
    case IR_B: return 3;
    default: return 0;
  }
}

// index into eval_args of group g (0..2), of mix (-1) or of global (-2); -1 if absent
int arg_index(const r0hip_circuit_tables& t, int what) {
  for (size_t i = 0; i < t.n_eval_args; i++)
    if (t.eval_args[i] == what) return int(i);
  return -1;
}

std::string validate_ir(const r0hip_circuit_tables& t) {
  if (!t.ir) return "ir: NULL";
  if (t.n_ir == 0) return "n_ir: 0 records";
  if (t.n_ir > kMaxIr) return "n_ir: " + str(t.n_ir) + " records exceed the cap of " + str(kMaxIr);
  const Tap* taps = reinterpret_cast<const Tap*>(t.taps);
  std::vector<uint8_t> type(t.n_ir, 0);
  for (size_t k = 0; k < t.n_ir; k++) {
    const uint32_t* r = t.ir + 6 * k;
    const std::string at = "ir: record " + str(k) + ": ";
    const uint32_t op = r[0];
    if (op > IR_R) return at + "op " + str(op) + " is not one of \"celg+-*abr\"";
    if (op == IR_R) {
      if (k + 1 != t.n_ir) return at + "the r record is not last";
      if (r[1] >= k) return at + "r names value " + str(r[1]) + " before it is made";
      continue;
    }
    if (k + 1 == t.n_ir) return at + "the last record is not the r record";
    if (r[1] != k) return at + "dst " + str(r[1]) + " is not the next dense id " + str(k);
    for (int j = 0; j < n_id_operands(op); j++)
      if (r[2 + j] >= r[1]) return at + "operand id " + str(r[2 + j]) + " is not below dst " + str(r[1]);
    switch (op) {
      case IR_C:
        if (r[2] >= kPrime) return at + "c: the constant word is not below p";
        break;
      case IR_E:
        for (int j = 0; j < 4; j++)
          if (r[2 + j] >= kPrime) return at + "e: a constant word is not below p";
        type[k] = 1;
        break;
      case IR_L:
        if (r[2] >= t.n_taps) return at + "l: tap index " + str(r[2]) + " is not below n_taps " + str(t.n_taps);
        if (arg_index(t, int(taps[r[2]].group)) < 0)
          return at + "l: tap " + str(r[2]) + " is of group " + str(taps[r[2]].group) +
                 ", which eval_args does not have as a register group";
        break;
      case IR_G: {
        if (r[2] > 1) return at + "g: " + str(r[2]) + " is neither 0 (mix) nor 1 (global)";
        if (arg_index(t, r[2] ? -2 : -1) < 0)
          return at + "g: eval_args has no " + std::string(r[2] ? "global" : "mix") + " argument";
        const size_t lim = r[2] ? t.output_size : t.mix_size;
        if (r[3] >= lim)
          return at + "g: word " + str(r[3]) + " is not below " + (r[2] ? "output_size " : "mix_size ") + str(lim);
        break;
      }
      case IR_ADD: case IR_SUB: case IR_MUL:
        type[k] = type[r[2]] | type[r[3]];
        break;
      case IR_A: case IR_B: {
        const uint32_t pw = r[op == IR_A ? 4 : 5];
        if (pw >= t.n_poly_mix)
          return at + "power index " + str(pw) + " is not below n_poly_mix " + str(t.n_poly_mix);
        if (!type[r[2]]) return at + "the ACC operand " + str(r[2]) + " is an Fp value, not an FpExt";
        type[k] = 1;
        break;
      }
    }
  }
  return "";
}

}  // namespace

std::string validate(const r0hip_circuit_tables& t) {
  // the name
  if (!t.name) return "name: NULL";
  const std::string name = t.name;
  if (name.empty() || name.size() > kMaxName) return "name: not 1 to " + str(kMaxName) + " characters";
  for (size_t i = 0; i < name.size(); i++) {
    const char ch = name[i];
    const bool alpha = (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || ch == '_';
    if (!(alpha || (i > 0 && ch >= '0' && ch <= '9'))) return "name: not a C identifier";
  }
  // the taps
  if (!t.taps || t.n_taps == 0) return "taps: none";
  if (t.n_taps >= (size_t(1) << 31)) return "n_taps: too many";
  const Tap* taps = reinterpret_cast<const Tap*>(t.taps);
  auto key = [&](size_t i) { return std::make_tuple(taps[i].group, taps[i].offset, taps[i].back); };
  auto reg = [&](size_t i) { return std::make_tuple(taps[i].group, taps[i].offset); };
  for (size_t i = 0; i < t.n_taps; i++) {
    if (taps[i].group > 2) return "taps: entry " + str(i) + ": group " + str(taps[i].group) + " is not 0, 1 or 2";
    if (i && !(key(i - 1) < key(i)))
      return "taps: entry " + str(i) + " is not sorted by group, offset and back after entry " + str(i - 1);
  }
  // skip: the taps of one register are adjacent and carry the register's tap count
  std::vector<std::pair<size_t, size_t>> regs;
  for (size_t cur = 0; cur < t.n_taps;) {
    const size_t sk = taps[cur].skip;
    if (sk < 1 || sk > t.n_taps - cur)
      return "taps: entry " + str(cur) + ": skip " + str(sk) + " does not tile the registers";
    for (size_t j = cur; j < cur + sk; j++)
      if (taps[j].skip != sk || reg(j) != reg(cur))
        return "taps: entry " + str(j) + ": skip " + str(taps[j].skip) + " does not tile the registers";
    if (cur + sk < t.n_taps && reg(cur + sk) == reg(cur))
      return "taps: entry " + str(cur + sk) + ": skip " + str(sk) + " of entry " + str(cur) +
             " does not tile the registers";
    regs.push_back({cur, sk});
    cur += sk;
  }
  // combos
  if (!t.combo_begin || (!t.combo_taps && t.n_combo_taps)) return "combo_begin: NULL";
  if (t.combos_count == 0 || t.combos_count >= (size_t(1) << 31)) return "combos_count: not a count of combos";
  {
    const uint32_t* cb = t.combo_begin;
    bool ok = cb[0] == 0 && cb[t.combos_count] == t.n_combo_taps;
    for (size_t i = 0; ok && i < t.combos_count; i++) ok = cb[i] < cb[i + 1];
    if (!ok)
      return "combo_begin: is not " + str(t.combos_count) + " + 1 rising offsets into the " + str(t.n_combo_taps) +
             " combo_taps";
    for (auto [cur, sk] : regs) {
      const uint32_t c = taps[cur].combo;
      for (size_t j = cur; j < cur + sk; j++)
        if (taps[j].combo != c || c >= t.combos_count)
          return "combo_begin: register of tap " + str(cur) + ": combo " + str(taps[j].combo) + " is not one of " +
                 str(t.combos_count);
      bool same = cb[c + 1] - cb[c] == sk;
      for (size_t j = 0; same && j < sk; j++) same = t.combo_taps[cb[c] + j] == taps[cur + j].back;
      if (!same) return "combo_begin: combo " + str(c) + " disagrees with the backs of the register of tap " + str(cur);
    }
  }
  // groups
  if (t.n_groups != 3) return "n_groups: " + str(t.n_groups) + " is not 3 (accum, code, data)";
  if (!t.group_begin) return "group_begin: NULL";
  if (!t.group_sizes) return "group_sizes: NULL";
  for (uint32_t g = 0; g <= 3; g++) {
    size_t want = 0;
    for (size_t i = 0; i < t.n_taps; i++) want += g > 0 && taps[i].group < g;
    if (t.group_begin[g] != want)
      return "group_begin: entry " + str(g) + " is " + str(t.group_begin[g]) + ", the taps give " + str(want);
  }
  for (uint32_t g = 0; g < 3; g++) {
    // sorted taps: the group's offsets must run 0, 1, .. without a gap
    uint32_t cols = 0;
    for (size_t i = t.group_begin[g]; i < t.group_begin[g + 1]; i++) {
      if (taps[i].offset > cols) return "group_sizes: group " + str(g) + ": the taps' offsets skip column " + str(cols);
      if (taps[i].offset == cols) cols++;
    }
    if (cols == 0) return "group_sizes: group " + str(g) + " has no tap";
    if (t.group_sizes[g] != cols)
      return "group_sizes: group " + str(g) + " is " + str(t.group_sizes[g]) + ", the taps give " + str(cols);
  }
  if (!t.poly_mix_powers && t.n_poly_mix) return "poly_mix_powers: NULL";
  if (t.mix_size >= kMaxWords) return "mix_size: " + str(t.mix_size) + " is not below " + str(kMaxWords);
  if (t.output_size >= kMaxWords) return "output_size: " + str(t.output_size) + " is not below " + str(kMaxWords);
  if (!t.eval_args || t.n_eval_args == 0 || t.n_eval_args > kMaxEvalArgs)
    return "eval_args: not 1 to " + str(kMaxEvalArgs) + " arguments";
  for (size_t i = 0; i < t.n_eval_args; i++)
    if (t.eval_args[i] < -2 || t.eval_args[i] > 2)
      return "eval_args: entry " + str(i) + " is " + std::to_string(t.eval_args[i]) +
             ", not 0 accum, 1 code, 2 data, -1 mix or -2 global";
  return validate_ir(t);
}

std::vector<uint8_t> infer_types(const uint32_t* ir, size_t n_ir) {
  std::vector<uint8_t> type(n_ir, 0);
  for (size_t k = 0; k < n_ir; k++) {
    const uint32_t* r = ir + 6 * k;
    switch (r[0]) {
      case IR_E: case IR_A: case IR_B: type[k] = 1; break;
      case IR_ADD: case IR_SUB: case IR_MUL: type[k] = type[r[2]] | type[r[3]]; break;
      default: break;
    }
  }
  return type;
}

Programs compile(const r0hip_circuit_tables& t) {
  Programs p;
  const size_t n = t.n_ir;
  const uint32_t* ir = t.ir;
  const std::vector<uint8_t> type = infer_types(ir, n);
  const Tap* taps = reinterpret_cast<const Tap*>(t.taps);
  for (size_t i = 0; i < t.n_taps; i++) {
    const uint32_t arg = uint32_t(arg_index(t, int(taps[i].group)));  // absent: no l names it
    p.taps_check.push_back(TapRef{arg, taps[i].offset, taps[i].back * 4u, 0});
    p.taps_rows.push_back(TapRef{arg, taps[i].offset, taps[i].back, 0});
  }
  // last use in program order; the r record reads its value too
  std::vector<uint32_t> last(n, 0);
  for (size_t k = 0; k < n; k++) {
    const uint32_t* r = ir + 6 * k;
    for (int j = 0; j < n_id_operands(r[0]); j++) last[r[2 + j]] = uint32_t(k);
    if (r[0] == IR_R) last[r[1]] = uint32_t(k);
  }
  // a value's operand form: a leaf is read where it is used, a computed value from its slot
  std::vector<uint32_t> slot(n, 0), ext_const(n, 0);
  for (size_t k = 0; k < n; k++)
    if (ir[6 * k] == IR_E) {
      ext_const[k] = uint32_t(p.consts.size() / 4);
      p.consts.insert(p.consts.end(), ir + 6 * k + 2, ir + 6 * k + 6);
    }
  auto operand = [&](uint32_t id, uint32_t* value) -> uint32_t {
    const uint32_t* r = ir + 6 * size_t(id);
    switch (r[0]) {
      case IR_C: *value = r[2]; return K_FP_IMM;
      case IR_E: *value = ext_const[id]; return K_EXT_IMM;
      case IR_L: *value = r[2]; return K_TAP;
      case IR_G: *value = (uint32_t(arg_index(t, r[2] ? -2 : -1)) << 24) | r[3]; return K_WORD;
      default: *value = slot[id]; return type[id] ? K_EXT_SLOT : K_FP_SLOT;
    }
  };
  // two free lists, one per slot file; a slot is free again after its value's last use, and the
  // record that makes that use may take it for its own result (it reads before it writes)
  std::vector<uint32_t> free_list[2];
  uint32_t count[2] = {0, 0};
  auto release = [&](uint32_t id, size_t k) {
    if (ir[6 * size_t(id)] >= IR_ADD && last[id] == k) {
      free_list[type[id]].push_back(slot[id]);
      last[id] = uint32_t(n);  // once, also when the record names the value twice
    }
  };
  for (size_t k = 0; k < n; k++) {
    const uint32_t* r = ir + 6 * k;
    const uint32_t op = r[0];
    if (op < IR_ADD) continue;
    Record rec{};
    uint32_t kx = K_NONE, ky = K_NONE, ka = K_NONE;
    if (op == IR_R) {
      kx = operand(r[1], &rec.x);
      rec.op = B_RET * 4 + (kind_is_ext(kx) ? 1 : 0);
      rec.kinds = kx;
      p.code.push_back(rec);
      break;
    }
    Base base;
    if (op == IR_A || op == IR_B) {
      ka = operand(r[2], &rec.acc);
      kx = operand(r[3], &rec.x);
      if (op == IR_B) ky = operand(r[4], &rec.y);
      rec.k = r[op == IR_A ? 4 : 5];
      base = op == IR_A ? B_ACC_A : B_ACC_B;
    } else {
      kx = operand(r[2], &rec.x);
      ky = operand(r[3], &rec.y);
      base = op == IR_ADD ? B_ADD : (op == IR_SUB ? B_SUB : B_MUL);
    }
    const bool xe = kind_is_ext(kx), ye = kind_is_ext(ky);
    rec.op = base * 4 + (xe ? 1 : 0) + (ye ? 2 : 0);
    rec.kinds = kx | (ky << 4) | (ka << 8);
    // field multiplications: x * y, then (a, b) the product with the power
    if (base == B_MUL || base == B_ACC_B) p.modmuls += xe && ye ? 16 : (xe || ye ? 4 : 1);
    if (base == B_ACC_A) p.modmuls += xe ? 16 : 4;
    if (base == B_ACC_B) p.modmuls += xe || ye ? 16 : 4;
    for (int j = 0; j < n_id_operands(op); j++) release(r[2 + j], k);
    auto& fl = free_list[type[k]];
    if (fl.empty()) {
      slot[k] = count[type[k]]++;
    } else {
      slot[k] = fl.back();
      fl.pop_back();
    }
    rec.dst = slot[k];
    p.code.push_back(rec);
    if (last[k] == 0 && k != 0) {  // a value nothing reads: its slot is free at once
      fl.push_back(slot[k]);
      last[k] = uint32_t(n);
    }
  }
  p.n_fp_slots = count[0];
  p.n_ext_slots = count[1];
  return p;
}

}  // namespace rt
}  // namespace r0
