// Stand-alone check of the native recursion preflight (risc0_amd/csrc/recursion_preflight.cpp),
// built by tests/test_recursion_preflight_native.py with -fsanitize=address,undefined.
//
//   recursion_preflight_host CASES [FUZZ_PROGRAMS]
//
// CASES (written by tests/recursion_input_programs.write_cases): per case a line
// `name po2 n_code n_input` and a line of n_code code words then n_input input words. Each is
// decoded and run; one line per case goes to stdout, `name ok n_wom n_iops n_output hash` (FNV-1a
// over the cycles, WOM, IOP values and output, which the test recomputes from the C ABI's arrays)
// or `name err message`. Then FUZZ_PROGRAMS programs of random rows (random 23-word rows, and
// rows with a valid selector and random operands) are decoded in both forms and run on random
// input: each must be refused or run, and the sanitizers must stay silent. Exit status 0 unless a
// case file is malformed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "recursion_preflight.h"

namespace {

uint64_t fnv(uint64_t h, const std::vector<uint32_t>& v, size_t words) {
  for (size_t i = 0; i < words; i++)
    for (int b = 0; b < 4; b++) h = (h ^ ((v[i] >> (8 * b)) & 0xFF)) * 0x100000001B3ull;
  return h;
}

// decode and run; returns the report after the case's name
std::string run_case(const std::vector<uint32_t>& code, int form, uint32_t po2, const std::vector<uint32_t>& input) {
  try {
    const r0::rpf::Program p = r0::rpf::decode(code.data(), code.size(), form, po2);
    std::vector<uint32_t> wom(4 * p.n_wom + 1), iops(4 * p.n_iops + 1), out(p.n_output + 1);
    r0::rpf::run(p, input.data(), input.size(), wom.data(), iops.data(), out.data());
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv(h, p.cycles, p.cycles.size());
    h = fnv(h, wom, 4 * p.n_wom);
    h = fnv(h, iops, 4 * p.n_iops);
    h = fnv(h, out, p.n_output);
    return "ok " + std::to_string(p.n_wom) + " " + std::to_string(p.n_iops) + " " + std::to_string(p.n_output) + " " +
           std::to_string(h);
  } catch (const std::exception& e) {
    return std::string("err ") + e.what();
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s CASES [FUZZ_PROGRAMS]\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string name;
  uint32_t po2;
  size_t n_code, n_input;
  while (in >> name >> po2 >> n_code >> n_input) {
    std::vector<uint32_t> code(n_code), input(n_input);
    for (auto& w : code) in >> w;
    for (auto& w : input) in >> w;
    if (!in) {
      std::fprintf(stderr, "case %s is cut short\n", name.c_str());
      return 2;
    }
    std::cout << name << " " << run_case(code, 0, po2, input) << "\n";
  }

  const int fuzz = argc > 2 ? std::atoi(argv[2]) : 0;
  std::mt19937_64 rng(0x5249534330ull);
  constexpr uint32_t kP = 0x78000001u;
  size_t ran = 0, refused = 0;
  for (int t = 0; t < fuzz; t++) {
    const size_t rows = 1 + rng() % 64;
    std::vector<uint32_t> code(23 * rows);
    const int style = t % 3;  // 0: any words; 1: small words; 2: a valid selector, small operands
    for (size_t r = 0; r < rows; r++) {
      uint32_t* w = &code[23 * r];
      for (int c = 0; c < 23; c++) w[c] = style == 0 ? uint32_t(rng()) : uint32_t(rng() % (style == 1 ? 3 : 40));
      if (style == 2) {
        for (int c = 1; c <= 7; c++) w[c] = 0;
        w[1 + rng() % 6] = 1;  // never checked_bytes (column 7), which decode refuses
        if (w[1] == 1)
          for (int i = 0; i < 3; i++) w[8 + 4 * i] = uint32_t(rng() % 12);
        if (rng() % 8 == 0) w[0] = uint32_t(rng());  // a far write address now and then
      }
    }
    std::vector<uint32_t> input(rng() % 64);
    for (auto& w : input) w = uint32_t(rng());
    for (int form = 0; form < 2; form++) {
      std::vector<uint32_t> c = code;
      if (form == 1 && t % 2)
        for (auto& w : c) w %= kP;  // else most programs are refused as non-canonical: that path too
      const std::string res = run_case(c, form, 11 + uint32_t(t % 3), input);
      (res[0] == 'o' ? ran : refused)++;
    }
  }
  if (fuzz) std::cout << "fuzz " << fuzz << " programs: " << ran << " ran, " << refused << " refused\n";
  return 0;
}
