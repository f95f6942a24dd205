// Host check of vfy::hash_tops (risc0_amd/csrc/verify_core.h), the level-by-level hashing of a
// Merkle verifier's top layer that the device receipt check of Poseidon254 seals can use
// (R0_VERIFY_P254_TOPS=1; the serial loop is the default): for top sizes
// 1, 2, 4 and 32 and 1, 3 and 8 threads it must fill exactly the rest[] of the reference's serial
// loop (rest[i] for 1 <= i < top size), for every suite, on random digests and on the BN254 edge
// digests 0, r - 1, r and 2^256 - 1; and a Poseidon2 top layer with a word >= p must throw what
// the serial loop throws. Stand-alone: built by tests/test_verify_p254_host.py with g++, also under
// -fsanitize=address,undefined. Prints OK and returns 0 when everything matches.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "verify_core.h"

using namespace r0;
using namespace r0::vfy;

// merkle.rs:105-118 as MerkleVerifier's constructor has it
static std::vector<Digest> serial(int suite, const std::vector<Digest>& top) {
  const size_t top_size = top.size();
  std::vector<Digest> rest(top_size, Digest{});
  for (size_t i = top_size; i-- > top_size / 2 && i >= 1;)
    rest[i] = hash_pair(suite, top[2 * i - top_size], top[2 * i + 1 - top_size]);
  for (size_t i = top_size / 2; i-- > 1;) rest[i] = hash_pair(suite, rest[2 * i], rest[2 * i + 1]);
  return rest;
}

static int failures = 0;

static void compare(int suite, const std::vector<Digest>& top, const char* what) {
  const std::vector<Digest> want = serial(suite, top);
  for (unsigned threads : {1u, 3u, 8u}) {
    std::vector<Digest> got(3, digest_of(top[0].w));  // stale contents must not survive
    hash_tops(suite, top, threads, got);
    bool ok = got.size() == want.size();
    for (size_t i = 1; ok && i < want.size(); i++) ok = same(got[i], want[i]);
    if (!ok) {
      std::printf("MISMATCH suite %d top %zu threads %u (%s)\n", suite, top.size(), threads, what);
      failures++;
    }
  }
}

int main() {
  std::mt19937_64 rng(0x70323534);
  // r, little-endian words (bn254.h's kMod packed back into 32-bit words)
  uint32_t r_words[8], rm1[8], ones[8], zero[8] = {0};
  bn::Fr mod;
  for (int i = 0; i < 9; i++) mod.l[i] = bn::kMod[i];
  bn::to_words(mod, r_words);
  for (int i = 0; i < 8; i++) rm1[i] = r_words[i], ones[i] = 0xFFFFFFFFu;
  rm1[0] -= 1;  // r is odd
  const uint32_t* edges[4] = {zero, rm1, r_words, ones};
  for (int suite = 0; suite < 3; suite++) {
    for (size_t top_size : {size_t(1), size_t(2), size_t(4), size_t(32)}) {
      std::vector<Digest> top(top_size);
      for (auto& d : top)
        for (auto& w : d.w) w = suite == 0 ? uint32_t(rng() % kP) : uint32_t(rng());
      compare(suite, top, "random");
      if (suite == 0) continue;  // the edge digests have words >= p
      for (size_t i = 0; i < top_size; i++) top[i] = digest_of(edges[(i + i / 4) % 4]);
      compare(suite, top, "edges");
    }
  }
  // Poseidon2: a word >= p in the top layer is refused with the serial loop's message
  for (size_t at : {size_t(0), size_t(13), size_t(31)}) {
    std::vector<Digest> top(32);
    for (auto& d : top)
      for (auto& w : d.w) w = uint32_t(rng() % kP);
    top[at].w[3] = kP;
    std::string want, got;
    try {
      serial(0, top);
    } catch (const std::exception& e) {
      want = e.what();
    }
    for (unsigned threads : {1u, 3u, 8u}) {
      std::vector<Digest> rest;
      got.clear();
      try {
        hash_tops(0, top, threads, rest);
      } catch (const std::exception& e) {
        got = e.what();
      }
      if (want.empty() || got != want) {
        std::printf("MISMATCH error at %zu threads %u: '%s' against '%s'\n", at, threads, got.c_str(), want.c_str());
        failures++;
      }
    }
  }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
