// The circuits a process knows: those compiled in (gen/circuits.cpp) and, after them, those
// handed over at run time through r0hip_circuit_register. Host code only.
// A registration validates the tables (circuit_rt.cpp), copies them, compiles the constraint
// program to the interpreter's bytecode and appends a CircuitDef to a fixed table. Writers
// serialise on a mutex; the entry is complete before the count is raised with release order, and
// readers load the count with acquire order and never lock. Entries are never moved or freed:
// proofs hold `const CircuitDef*`.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/r0hip.h"
#include "circuit.h"
#include "circuit_rt.h"

namespace r0 {
namespace {

// the copies a registered CircuitDef points into
struct Registered {
  std::string name;
  std::vector<uint32_t> taps, combo_taps, combo_begin, group_begin, group_sizes, pm, ir;
  std::vector<int> eval_args;
  char info[16];
  rt::Programs programs;
  CircuitDef def;
};

const Registered* g_table[kMaxRegistered];
std::atomic<size_t> g_count{0};
std::mutex g_write;

std::vector<uint32_t> copy_words(const uint32_t* p, size_t n) { return std::vector<uint32_t>(p, p + n); }

}  // namespace

size_t circuit_count() { return compiled_circuit_count() + g_count.load(std::memory_order_acquire); }

const CircuitDef& circuit_at(size_t i) {
  const size_t nc = compiled_circuit_count();
  return i < nc ? compiled_circuit_at(i) : g_table[i - nc]->def;
}

const CircuitDef* find_circuit(const std::string& name) {
  if (const CircuitDef* c = compiled_find_circuit(name)) return c;
  const size_t n = g_count.load(std::memory_order_acquire);
  for (size_t i = 0; i < n; i++)
    if (g_table[i]->name == name) return &g_table[i]->def;
  return nullptr;
}

std::string unknown_circuit(const char* name) {
  std::string m = std::string("unknown circuit ") + (name ? name : "(null)") + " (compiled in: ";
  const size_t nc = compiled_circuit_count(), n = circuit_count();
  for (size_t i = 0; i < nc; i++) m += (i ? ", " : "") + std::string(compiled_circuit_at(i).name);
  for (size_t i = nc; i < n; i++) m += (i == nc ? "; registered: " : ", ") + std::string(circuit_at(i).name);
  return m + ")";
}

namespace {

void register_circuit(const r0hip_circuit_tables* t, size_t t_size) {
  const std::string who = "r0hip_circuit_register: ";
  auto require = [&](bool ok, const std::string& m) {
    if (!ok) throw std::runtime_error("r0hip: " + who + m);
  };
  require(t != nullptr, "t is NULL");
  require(t_size == sizeof(r0hip_circuit_tables), "t_size: " + std::to_string(t_size) +
                                                      " is not sizeof(r0hip_circuit_tables) = " +
                                                      std::to_string(sizeof(r0hip_circuit_tables)));
  const std::string bad = rt::validate(*t);
  require(bad.empty(), bad);
  // everything that can throw happens before the table is touched
  auto r = std::make_unique<Registered>();
  r->name = t->name;
  r->taps = copy_words(t->taps, 5 * t->n_taps);
  r->combo_taps = copy_words(t->combo_taps, t->n_combo_taps);
  r->combo_begin = copy_words(t->combo_begin, t->combos_count + 1);
  r->group_begin = copy_words(t->group_begin, t->n_groups + 1);
  r->group_sizes = copy_words(t->group_sizes, t->n_groups);
  r->pm = copy_words(t->poly_mix_powers, t->n_poly_mix);
  r->ir = copy_words(t->ir, 6 * t->n_ir);
  r->eval_args.assign(t->eval_args, t->eval_args + t->n_eval_args);
  memcpy(r->info, t->info, 16);
  r->programs = rt::compile(*t);
  CircuitDef& d = r->def;
  d = CircuitDef{};
  d.name = r->name.c_str();
  d.taps = r->taps.data();
  d.n_taps = t->n_taps;
  d.combo_taps = r->combo_taps.data();
  d.n_combo_taps = t->n_combo_taps;
  d.combo_begin = r->combo_begin.data();
  d.combos_count = t->combos_count;
  d.group_begin = r->group_begin.data();
  d.n_groups = t->n_groups;
  d.group_sizes = r->group_sizes.data();
  d.poly_mix_powers = r->pm.data();
  d.n_poly_mix = t->n_poly_mix;
  d.circuit_info = r->info;
  d.mix_size = t->mix_size;
  d.output_size = t->output_size;
  d.eval_args = r->eval_args.data();
  d.n_eval_args = t->n_eval_args;
  d.ir = r->ir.data();
  d.n_ir = t->n_ir;
  d.interp = &r->programs;
  std::lock_guard<std::mutex> lk(g_write);
  require(find_circuit(r->name) == nullptr, "name: " + r->name + " is taken");
  const size_t n = g_count.load(std::memory_order_relaxed);
  require(n < kMaxRegistered, "the registry is full (" + std::to_string(kMaxRegistered) + " circuits)");
  g_table[n] = r.release();
  g_count.store(n + 1, std::memory_order_release);
}

}  // namespace
}  // namespace r0

extern "C" const char* r0hip_circuit_register(const r0hip_circuit_tables* t, size_t t_size) {
  try {
    r0::register_circuit(t, t_size);
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}
