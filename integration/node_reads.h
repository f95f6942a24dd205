// How the per-op driver answers get_at on a Merkle node heap (hal_prover.cpp Buf::at, the same
// logic as integration/rust/hal_hip.rs): a page-locked host mirror of the whole heap while the
// process's mirrors fit under a budget, and otherwise one r0hip_merkle_paths_host call per
// opening, whose nodes a small per-buffer cache hands to the get_at calls that follow.
//
// Host code only. It makes three r0hip_* calls (r0hip_host_alloc, r0hip_host_free,
// r0hip_merkle_paths_host), so tests/native/node_reads_host.cpp runs it against host stubs of
// those three under the address and undefined-behaviour sanitizers.
#ifndef R0HIP_NODE_READS_H
#define R0HIP_NODE_READS_H
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/r0hip.h"

namespace halp {

// Process-wide count of the page-locked bytes that live mirrors hold, and what became of every
// mirror and node read since the last reset (halp_mirror_stats).
struct MirrorLedger {
  static constexpr uint64_t kDefaultBudget = uint64_t(4) << 30;  // 4 GiB: every proof up to po2 21 mirrors all trees
  std::atomic<uint64_t> budget{kDefaultBudget};
  std::atomic<uint64_t> live{0}, peak{0}, started{0}, refused{0}, fetches{0}, hits{0};

  // A page-locked block of `bytes` for a mirror, or nullptr when the live mirrors plus this one
  // would pass the budget or the allocation fails: both are one refusal, never an error.
  void* acquire(uint64_t bytes) {
    const uint64_t cap = budget.load();
    uint64_t cur = live.load();
    do {
      if (bytes > cap || cur > cap - bytes) {
        refused++;
        return nullptr;
      }
    } while (!live.compare_exchange_weak(cur, cur + bytes));
    void* h = nullptr;
    if (const char* err = r0hip_host_alloc(&h, bytes)) {
      free(const_cast<char*>(err));
      live -= bytes;
      refused++;
      return nullptr;
    }
    uint64_t top = peak.load();
    while (top < cur + bytes && !peak.compare_exchange_weak(top, cur + bytes)) {
    }
    return h;
  }
  void release(void* h, uint64_t bytes) {
    free(const_cast<char*>(r0hip_host_free(h)));  // a drop never fails the proof
    live -= bytes;
  }
  void reset_stats() {
    started = refused = fetches = hits = 0;
    peak = live.load();
  }
  void stats(uint64_t out[5]) const {
    out[0] = started, out[1] = refused, out[2] = fetches, out[3] = hits, out[4] = peak;
  }
};
inline MirrorLedger& ledger() {
  static MirrorLedger l;
  return l;
}

// The nodes of the last opening fetched from an un-mirrored heap. MerkleTreeProver::prove
// (merkle.rs:131-138) reads node j, then (j >> k) ^ 1 for k = 1, 2, ..: the first read misses and
// fetches all of them in one call (entry k of the path is keyed by (j, k)), the rest hit.
struct PathCache {
  uint64_t j = 0;     // 0: empty (node 0 is not a node)
  size_t levels = 0;
  std::vector<uint32_t> words;  // levels x 8
  void clear() { j = 0; }
  // floor(log2 j) nodes: j and every sibling up to the root's children; the root's children
  // themselves (j < 4) are a path of one
  static size_t levels_of(uint64_t node) {
    size_t l = 0;
    while (node >> (l + 1)) l++;
    return l < 2 ? 1 : l;
  }
  const uint32_t* find(uint64_t node) const {
    if (!j) return nullptr;
    if (node == j) return words.data();
    for (size_t k = 1; k < levels; k++)
      if (node == ((j >> k) ^ 1)) return words.data() + k * 8;
    return nullptr;
  }
  // the digest of `node` (>= 2) of the device heap d_nodes, from the cache or one device call
  const uint32_t* get(const uint32_t* d_nodes, size_t heap_digests, uint64_t node) {
    if (const uint32_t* w = find(node)) {
      ledger().hits++;
      return w;
    }
    clear();
    const size_t l = levels_of(node);
    words.resize(l * 8);
    if (const char* err = r0hip_merkle_paths_host(words.data(), d_nodes, heap_digests, &node, 1, l)) {
      std::string m(err);
      free(const_cast<char*>(err));
      throw std::runtime_error(m);
    }
    ledger().fetches++;
    j = node;
    levels = l;
    return words.data();
  }
};

}  // namespace halp
#endif  // R0HIP_NODE_READS_H
