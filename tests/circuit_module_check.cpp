// Stand-alone check of the host logic of r0hip_circuit_load (risc0_amd/csrc/circuit_module.cpp
// with the table validator of circuit_rt.cpp), built by tests/test_circuit_module_host.py with
// -fsanitize=address,undefined and run as a program of its own. It links no HIP: descriptors are
// made in memory from a tables file, with info functions of this program in place of kernels.
//   circuit_module_check <tables>
// runs every case below and prints "<case>: ok" for an accepted descriptor or "<case>: <refusal>";
// the exit status is 1 when a case did not end as the table says (a substring of the refusal, ""
// for acceptance).
// <tables>: the text format of tests/circuit_rt_check.cpp, lines "<key> <count> <values...>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "circuit_module.h"

using namespace r0;

struct Loaded {
  std::string name;
  std::map<std::string, std::vector<int64_t>> v;
  std::vector<uint32_t> u32[8];
  std::vector<int32_t> args;
  r0hip_circuit_tables t{};
};

static const std::vector<uint32_t>& words(Loaded& L, int slot, const char* key) {
  L.u32[slot].clear();
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
}

// the tables struct over L's vectors (again after a case edited them)
static void bind(Loaded& L) {
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
  L.args.clear();
  for (int64_t x : L.v["eval_args"]) L.args.push_back(int32_t(x));
  t.eval_args = L.args.data();
  t.n_eval_args = L.args.size();
  t.ir = words(L, 6, "ir").data();
  t.n_ir = one("n_ir");
}

// ---- the kernels' view, served by this program ----
// exactly sized arrays on the heap, so that a check that reads one entry too many is an
// AddressSanitizer report
struct View {
  std::vector<int> combos, col_arg, col_idx;
  EvalCheckInfo info{};
  void finish() {
    info.combos = combos.data();
    info.col_arg = col_arg.data();
    info.col_idx = col_idx.data();
    info.ncols = int(col_arg.size());
  }
};
static View g_view[2];  // info(), rows_info()
static void uniform_stub(const uint32_t* const*, const uint32_t*, uint32_t*) {}
static void info_fn(EvalCheckInfo* out) { *out = g_view[0].info; }
static void rows_info_fn(EvalCheckInfo* out) { *out = g_view[1].info; }
static void launch_stub() {}

// a view that fits the tables: every column of every group argument, two folded products
static View good_view(const r0hip_circuit_tables& t) {
  View v;
  v.info.nargs = int(t.n_eval_args);
  v.info.npm = int(t.n_poly_mix);
  v.info.mat_fp = 3;
  v.info.mat_ext = 1;
  v.info.kernels = 2;
  v.info.modmuls_per_point = 10;
  v.info.n_uniform = 1;
  v.info.uniform = uniform_stub;
  v.combos = {2, 0, int(t.n_poly_mix) - 1, 1, 1};
  v.info.ncombos = 2;
  for (size_t a = 0; a < t.n_eval_args; a++)
    if (t.eval_args[a] >= 0)
      for (uint32_t c = 0; c < t.group_sizes[t.eval_args[a]]; c++) {
        v.col_arg.push_back(int(a));
        v.col_idx.push_back(int(c));
      }
  v.finish();
  return v;
}

struct Case {
  const char* id;
  const char* want;  // substring of the refusal, "" = accepted
  std::function<void(r0hip_module_desc&, Loaded&)> edit;
};

int main(int argc, char** argv) {
  if (argc != 2) {
    std::cerr << "usage: circuit_module_check <tables>\n";
    return 2;
  }
  Loaded base;
  load(argv[1], base);
  bind(base);
  const int group_arg = [&] {
    for (size_t a = 0; a < base.t.n_eval_args; a++)
      if (base.t.eval_args[a] == 2) return int(a);
    return -1;
  }();
  if (group_arg < 0 || base.t.n_poly_mix < 2) {
    std::cerr << "the tables have no data argument\n";
    return 2;
  }
  auto view = [](int k) -> View& { return g_view[k]; };
  const std::vector<Case> cases = {
      {"good", "", [](r0hip_module_desc&, Loaded&) {}},
      {"abi", "abi: the module has 2 for R0HIP_MODULE_ABI, the library 1", [](r0hip_module_desc& d, Loaded&) { d.abi = 2; }},
      {"desc_size", "desc_size: the module has", [](r0hip_module_desc& d, Loaded&) { d.desc_size += 8; }},
      {"args_size", "for sizeof(EvalCheckArgs), the library", [](r0hip_module_desc& d, Loaded&) { d.args_size -= 8; }},
      {"info_size", "for sizeof(EvalCheckInfo), the library", [](r0hip_module_desc& d, Loaded&) { d.info_size += 4; }},
      {"arch", "arch: the module was compiled for gfx942, the library for gfx950",
       [](r0hip_module_desc& d, Loaded&) { d.arch = "gfx942"; }},
      {"arch_null", "arch: NULL", [](r0hip_module_desc& d, Loaded&) { d.arch = nullptr; }},
      {"no_rows_info", "rows_info: NULL", [](r0hip_module_desc& d, Loaded&) { d.rows_info = nullptr; }},
      {"taps_unsorted", "taps: entry 1 is not sorted",
       [](r0hip_module_desc&, Loaded& L) {
         for (int k = 0; k < 5; k++) std::swap(L.v["taps"][k], L.v["taps"][5 + k]);
       }},
      {"ir_operand", "ir: record 5: operand id 5 is not below dst 5",
       [](r0hip_module_desc&, Loaded& L) { L.v["ir"][6 * 5 + 2] = 5; }},
      {"name", "name: not a C identifier", [](r0hip_module_desc&, Loaded& L) { L.name = "2fast"; }},
      {"nargs", "info(): nargs: the kernels take 4 arguments, eval_args has 5",
       [&](r0hip_module_desc&, Loaded&) { view(0).info.nargs = 4; }},
      {"rows_nargs", "rows_info(): nargs: the kernels take 6 arguments",
       [&](r0hip_module_desc&, Loaded&) { view(1).info.nargs = 6; }},
      {"col_idx", "info(): col_idx: column 0 is column 3 of",
       [&](r0hip_module_desc&, Loaded& L) {
         View& v = view(0);
         v.col_arg[0] = group_arg;
         v.col_idx[0] = int(L.t.group_sizes[2]);
       }},
      {"col_idx_negative", "col_idx: column 1 is column -1 of", [&](r0hip_module_desc&, Loaded&) { view(0).col_idx[1] = -1; }},
      {"col_arg", "rows_info(): col_arg: column 2 names argument 5 of 5",
       [&](r0hip_module_desc&, Loaded&) { view(1).col_arg[2] = 5; }},
      {"col_of_mix", "is column 1 of mix, which has 1",
       [&](r0hip_module_desc&, Loaded& L) {
         for (size_t a = 0; a < L.t.n_eval_args; a++)
           if (L.t.eval_args[a] == -1) view(0).col_arg[0] = int(a);
         view(0).col_idx[0] = 1;
       }},
      {"combo_index", "combos: product 0: power index 8 is not below npm 8",
       [&](r0hip_module_desc&, Loaded& L) { view(0).combos[2] = int(L.t.n_poly_mix); }},
      {"combo_count", "combos: product 1 has 0 factors", [&](r0hip_module_desc&, Loaded&) { view(0).combos[3] = 0; }},
      {"npm", "npm: the kernels index 9 poly_mix powers, poly_mix_powers has 8",
       [&](r0hip_module_desc&, Loaded& L) { view(0).info.npm = int(L.t.n_poly_mix) + 1; }},
      {"mat_fp", "mat_fp: -1 is not 0 to", [&](r0hip_module_desc&, Loaded&) { view(0).info.mat_fp = -1; }},
      {"mat_ext", "mat_ext: 65537 is not 0 to 65536", [&](r0hip_module_desc&, Loaded&) { view(1).info.mat_ext = 65537; }},
      {"kernels", "kernels: 65 is not 1 to 64", [&](r0hip_module_desc&, Loaded&) { view(0).info.kernels = 65; }},
      {"kernels_zero", "kernels: 0 is not 1 to 64", [&](r0hip_module_desc&, Loaded&) { view(1).info.kernels = 0; }},
      {"ncols_negative", "ncols: -1 is not", [&](r0hip_module_desc&, Loaded&) { view(0).info.ncols = -1; }},
      {"uniform_null", "uniform: NULL with n_uniform 1", [&](r0hip_module_desc&, Loaded&) { view(0).info.uniform = nullptr; }},
      {"no_columns_no_combos", "",
       [&](r0hip_module_desc&, Loaded&) {
         for (int k = 0; k < 2; k++) {
           View& v = view(k);
           v.combos.clear();
           v.col_arg.clear();
           v.col_idx.clear();
           v.info.ncombos = 0;
           v.finish();
         }
       }},
  };
  int failed = 0;
  for (const Case& c : cases) {
    Loaded L = base;
    bind(L);
    r0hip_module_desc d{};
    d.abi = R0HIP_MODULE_ABI;
    d.desc_size = uint32_t(sizeof(r0hip_module_desc));
    d.args_size = uint32_t(sizeof(EvalCheckArgs));
    d.info_size = uint32_t(sizeof(EvalCheckInfo));
    d.arch = "gfx950";
    d.eval_check = d.constraint_rows = launch_stub;
    d.info = reinterpret_cast<r0hip_module_fn>(&info_fn);
    d.rows_info = reinterpret_cast<r0hip_module_fn>(&rows_info_fn);
    g_view[0] = good_view(L.t);
    g_view[1] = good_view(L.t);
    g_view[0].finish();  // the pointers follow the vectors into their new home
    g_view[1].finish();
    c.edit(d, L);
    bind(L);  // the case may have edited the vectors the tables point into
    d.tables = L.t;
    const std::string got = mod::check_module(&d, mod::expect_here("gfx950"));
    std::cout << c.id << ": " << (got.empty() ? "ok" : got) << "\n";
    const bool as_wanted = *c.want ? got.find(c.want) != std::string::npos : got.empty();
    if (!as_wanted) {
      std::cout << "FAILED: " << c.id << ": wanted " << (*c.want ? c.want : "acceptance") << "\n";
      failed = 1;
    }
  }
  // a null descriptor
  const std::string none = mod::check_module(nullptr, mod::expect_here("gfx950"));
  std::cout << "null: " << none << "\n";
  if (none.find("no descriptor") == std::string::npos) failed = 1;
  return failed;
}
