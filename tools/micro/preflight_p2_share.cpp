// The host preflight of one recursion program on one thread, and how much of it its Poseidon2
// permutations are. No GPU, no HIP.
//   g++ -O3 -std=c++17 -I risc0_amd/csrc tools/micro/preflight_p2_share.cpp risc0_amd/csrc/recursion_preflight.cpp
//   ./a.out case.bin [warmups] [repeats]
// case.bin: u32 po2, n_code, n_input, then the code words (form 0) and the input words
// (tools/bench_recursion_input.py --p2-share writes it). Prints one JSON object:
//   preflight     rpf::run alone on the decoded program, ms per run
//   permutations  as many poseidon2_mix calls as the program has p2_partial rows, on one 24-word
//                 state fed from call to call (the preflight's own function and data dependence,
//                 without its loads and stores), ms for all of them
//   decode        rpf::decode, ms
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poseidon2.h"
#include "recursion_preflight.h"

namespace {
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void print(const char* name, std::vector<double> ms, const char* tail) {
  std::vector<double> s = ms;
  std::sort(s.begin(), s.end());
  std::printf("\"%s\": {\"ms\": [", name);
  for (size_t i = 0; i < ms.size(); i++) std::printf("%s%.3f", i ? ", " : "", ms[i]);
  std::printf("], \"median\": %.3f, \"min\": %.3f, \"max\": %.3f}%s", s[s.size() / 2], s.front(), s.back(), tail);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s case.bin [warmups] [repeats]\n", argv[0]);
    return 2;
  }
  const int warmups = argc > 2 ? std::atoi(argv[2]) : 2, repeats = argc > 3 ? std::max(1, std::atoi(argv[3])) : 7;
  std::FILE* f = std::fopen(argv[1], "rb");
  uint32_t head[3];
  if (!f || std::fread(head, 4, 3, f) != 3) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<uint32_t> code(head[1]), input(head[2]);
  if (std::fread(code.data(), 4, code.size(), f) != code.size() ||
      std::fread(input.data(), 4, input.size(), f) != input.size()) {
    std::fprintf(stderr, "%s is truncated\n", argv[1]);
    return 2;
  }
  std::fclose(f);
  using namespace r0::rpf;
  std::vector<double> t_decode, t_run, t_p2;
  Program p;
  for (int i = 0; i < warmups + repeats; i++) {
    const double t0 = now_ms();
    p = decode(code.data(), code.size(), 0, head[0]);
    if (i >= warmups) t_decode.push_back(now_ms() - t0);
  }
  size_t perms = 0;
  for (const Op& op : p.ops) perms += op.kind == kP2Partial;
  std::vector<uint32_t> wom(4 * p.n_wom + 4), iops(4 * p.n_iops + 4), output(p.n_output + 1);
  uint32_t sink = 0;
  for (int i = 0; i < warmups + repeats; i++) {
    double t0 = now_ms();
    run(p, input.data(), input.size(), wom.data(), iops.data(), output.data());
    if (i >= warmups) t_run.push_back(now_ms() - t0);
    sink ^= wom[4 * p.n_wom / 2];
    uint32_t st[24];
    for (int k = 0; k < 24; k++) st[k] = wom[k % (4 * p.n_wom + 1)] % 2013265921u;
    t0 = now_ms();
    for (size_t k = 0; k < perms; k++) r0::poseidon2_mix(st);
    if (i >= warmups) t_p2.push_back(now_ms() - t0);
    sink ^= st[0];
  }
  std::printf("{\"p2_permutations\": %zu, \"n_wom\": %zu, \"sink\": %u, ", perms, p.n_wom, sink);
  print("decode", t_decode, ", ");
  print("preflight", t_run, ", ");
  print("permutations", t_p2, "}\n");
  return 0;
}
