// The circuits a process knows: those compiled in (gen/circuits.cpp) and, after them, those
// handed over at run time through r0hip_circuit_register (tables: the device interprets the
// program) or r0hip_circuit_load (a circuit module: its own generated kernels). Host code only.
// A registration validates the tables (circuit_rt.cpp), copies them, compiles the constraint
// program to the interpreter's bytecode and appends a CircuitDef to a fixed table. Writers
// serialise on a mutex; the entry is complete before the count is raised with release order, and
// readers load the count with acquire order and never lock. Entries are never moved or freed:
// proofs hold `const CircuitDef*`.
// A load opens the module, passes its descriptor through the checks of circuit_module.cpp and
// appends a CircuitDef that points into the module: nothing is copied, the module owns its tables
// and is never closed once it is in the table. A refused module is closed again.
#include <dlfcn.h>

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
#include "circuit_module.h"
#include "circuit_rt.h"
#include "evalcheck.h"

// the architecture the library's kernels are compiled for (the Makefile's ARCH, handed over as a
// bare word)
#ifndef R0HIP_ARCH
#define R0HIP_ARCH gfx950
#endif
#define R0HIP_STR2(x) #x
#define R0HIP_STR(x) R0HIP_STR2(x)

namespace r0 {
namespace {

// the copies a registered CircuitDef points into; a loaded one points into its module and
// uses `name` and `def` only
struct Registered {
  int kind = 1;  // r0hip_circuit_backend: 1 interpreted, 2 a module
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

int circuit_backend(const std::string& name) {
  if (compiled_find_circuit(name)) return 0;
  const size_t n = g_count.load(std::memory_order_acquire);
  for (size_t i = 0; i < n; i++)
    if (g_table[i]->name == name) return g_table[i]->kind;
  return -1;
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

std::string load_module(const char* path) {
  auto require = [&](bool ok, const std::string& m) {
    if (!ok) throw std::runtime_error("r0hip: r0hip_circuit_load: " + m);
  };
  require(path != nullptr, "path is NULL");
  const std::string at = std::string(path) + ": ";
  dlerror();
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    const char* why = dlerror();
    require(false, at + (why ? why : "dlopen failed"));
  }
  // from here a refusal closes the handle again; dlopen counts, so a second load of a file
  // whose first load holds a registry entry leaves that one open
  struct Closer {
    void* h;
    ~Closer() {
      if (h) dlclose(h);
    }
  } closer{h};
  auto entry = reinterpret_cast<r0hip_module_entry_fn>(dlsym(h, R0HIP_MODULE_ENTRY));
  require(entry != nullptr, at + "no entry symbol " R0HIP_MODULE_ENTRY);
  const r0hip_module_desc* d = entry();
  const std::string bad = mod::check_module(d, mod::expect_here(R0HIP_STR(R0HIP_ARCH)));
  require(bad.empty(), at + bad);
  const r0hip_circuit_tables& t = d->tables;
  auto r = std::make_unique<Registered>();
  r->kind = 2;
  r->name = t.name;
  CircuitDef& c = r->def;
  c = CircuitDef{};
  c.name = t.name;
  c.taps = t.taps;
  c.n_taps = t.n_taps;
  c.combo_taps = t.combo_taps;
  c.n_combo_taps = t.n_combo_taps;
  c.combo_begin = t.combo_begin;
  c.combos_count = t.combos_count;
  c.group_begin = t.group_begin;
  c.n_groups = t.n_groups;
  c.group_sizes = t.group_sizes;
  c.poly_mix_powers = t.poly_mix_powers;
  c.n_poly_mix = t.n_poly_mix;
  c.circuit_info = reinterpret_cast<const char*>(t.info);
  c.mix_size = t.mix_size;
  c.output_size = t.output_size;
  c.eval_args = t.eval_args;
  c.n_eval_args = t.n_eval_args;
  c.eval_check = reinterpret_cast<void (*)(hipStream_t, const EvalCheckArgs&)>(d->eval_check);
  c.info = reinterpret_cast<void (*)(EvalCheckInfo*)>(d->info);
  c.constraint_rows = reinterpret_cast<void (*)(hipStream_t, const EvalCheckArgs&)>(d->constraint_rows);
  c.rows_info = reinterpret_cast<void (*)(EvalCheckInfo*)>(d->rows_info);
  c.ir = t.ir;
  c.n_ir = t.n_ir;
  std::lock_guard<std::mutex> lk(g_write);
  require(find_circuit(r->name) == nullptr, at + "name: " + r->name + " is taken");
  const size_t n = g_count.load(std::memory_order_relaxed);
  require(n < kMaxRegistered, at + "the registry is full (" + std::to_string(kMaxRegistered) + " circuits)");
  std::string name = r->name;
  g_table[n] = r.release();
  g_count.store(n + 1, std::memory_order_release);
  closer.h = nullptr;  // in the table: open for the life of the process
  return name;
}

}  // namespace
}  // namespace r0

extern "C" const char* r0hip_circuit_load(const char* path, char* name_out, size_t name_cap) {
  try {
    // a name has at most rt::kMaxName characters: a buffer that holds any name is asked for
    // before the file is opened, so no load succeeds without its name delivered
    if (name_out && name_cap <= r0::rt::kMaxName)
      throw std::runtime_error("r0hip: r0hip_circuit_load: name_cap " + std::to_string(name_cap) + " is below " +
                               std::to_string(r0::rt::kMaxName + 1));
    const std::string name = r0::load_module(path);
    if (name_out) memcpy(name_out, name.c_str(), name.size() + 1);
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}

extern "C" const char* r0hip_circuit_backend(const char* circuit, int* kind) {
  try {
    if (!kind) throw std::runtime_error("r0hip: r0hip_circuit_backend: kind is NULL");
    const int k = r0::circuit_backend(circuit ? circuit : "");
    if (k < 0) throw std::runtime_error("r0hip: r0hip_circuit_backend: " + r0::unknown_circuit(circuit));
    *kind = k;
    return nullptr;
  } catch (const std::exception& e) {
    return strdup(e.what());
  } catch (...) {
    return strdup("r0hip: unknown error");
  }
}

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
