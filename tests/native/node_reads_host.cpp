// integration/node_reads.h (the per-op driver's mirror budget and path cache) against host
// stubs of the three r0hip_* calls it makes, as a stand-alone program: built with
// -fsanitize=address,undefined by tests/test_mirror_budget_host.py. The "device" heap is a host
// array whose digest i holds the words 8i .. 8i+7, so every node a read returns names itself.
#include "../../integration/node_reads.h"

#include <cstdio>
#include <cstring>

namespace {
int g_allocs = 0, g_frees = 0, g_path_calls = 0;
bool g_fail_alloc = false;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      return 1;                                                \
    }                                                          \
  } while (0)
}  // namespace

extern "C" {
const char* r0hip_host_alloc(void** h_ptr, size_t bytes) {
  if (g_fail_alloc) return strdup("stub: no page-locked memory");
  g_allocs++;
  *h_ptr = malloc(bytes ? bytes : 1);
  return nullptr;
}
const char* r0hip_host_free(void* h_ptr) {
  g_frees++;
  free(h_ptr);
  return nullptr;
}
const char* r0hip_merkle_paths_host(uint32_t* h_dst, const uint32_t* d_nodes, size_t heap_digests,
                                    const uint64_t* h_idx, size_t n, size_t levels) {
  g_path_calls++;
  for (size_t i = 0; i < n; i++) {
    const uint64_t j = h_idx[i];
    if (j < 1 || j >= heap_digests || levels < 1 || (levels > 1 && (j >> (levels - 1)) < 2))
      return strdup("stub: bad index");
    for (size_t k = 0; k < levels; k++)
      memcpy(h_dst + (i * levels + k) * 8, d_nodes + (k == 0 ? j : ((j >> k) ^ 1)) * 8, 32);
  }
  return nullptr;
}
}

int main() {
  using namespace halp;
  MirrorLedger& L = ledger();
  uint64_t s[5];

  // --- the budget: refusals never fail, the peak never passes the budget ---
  CHECK(L.budget == (uint64_t(4) << 30));
  L.budget = 1000;
  void* a = L.acquire(600);
  CHECK(a && L.live == 600);
  CHECK(L.acquire(401) == nullptr && L.live == 600);  // would pass the budget
  void* b = L.acquire(400);                           // fits to the byte
  CHECK(b && L.live == 1000);
  CHECK(L.acquire(1) == nullptr);
  L.stats(s);
  CHECK(s[1] == 2 && s[4] == 1000);
  L.release(a, 600);
  CHECK(L.live == 400);
  g_fail_alloc = true;  // an allocation failure is a refusal too, and its error string is freed
  CHECK(L.acquire(100) == nullptr && L.live == 400);
  g_fail_alloc = false;
  L.stats(s);
  CHECK(s[1] == 3 && s[4] == 1000);
  L.reset_stats();
  L.stats(s);
  CHECK(s[0] == 0 && s[1] == 0 && s[2] == 0 && s[3] == 0 && s[4] == 400);  // the peak restarts from the live bytes
  L.release(b, 400);
  CHECK(L.live == 0 && g_allocs == 2 && g_frees == 2);
  L.budget = 0;
  void* z = L.acquire(0);  // nothing to pin always fits
  CHECK(z != nullptr);
  L.release(z, 0);
  CHECK(L.acquire(1) == nullptr);
  L.budget = ~uint64_t(0);
  void* c = L.acquire(64);
  CHECK(c && L.acquire(~uint64_t(0)) == nullptr);  // no wrap-around of live + bytes
  L.release(c, 64);
  L.reset_stats();

  // --- the path cache ---
  CHECK(PathCache::levels_of(2) == 1 && PathCache::levels_of(3) == 1 && PathCache::levels_of(4) == 2);
  CHECK(PathCache::levels_of(7) == 2 && PathCache::levels_of(8) == 3 && PathCache::levels_of((1u << 21) - 1) == 20);
  const size_t rows = 1 << 10, heap = 2 * rows;
  std::vector<uint32_t> nodes(heap * 8);
  for (size_t i = 0; i < nodes.size(); i++) nodes[i] = uint32_t(i);
  PathCache pc;
  // MerkleTreeProver::prove over three openings with top_size 32: idx += rows; while idx >= 64
  // read the sibling of idx, idx /= 2
  size_t reads = 0;
  for (size_t pos : {size_t(0), size_t(777), rows - 1}) {
    size_t idx = pos + rows;
    while (idx >= 64) {
      const size_t low = idx % 2;
      idx /= 2;
      const uint64_t node = 2 * idx + (1 - low);
      const uint32_t* w = pc.get(nodes.data(), heap, node);
      for (int k = 0; k < 8; k++) CHECK(w[k] == node * 8 + k);
      reads++;
    }
  }
  L.stats(s);
  CHECK(reads == 15 && g_path_calls == 3 && s[2] == 3 && s[3] == 12);  // one device call per opening
  // a written heap: the cache is dropped, the next read fetches again
  pc.clear();
  CHECK(pc.find(2 * rows - 2) == nullptr);
  nodes[(heap - 1) * 8] = 0xABCD;
  CHECK(pc.get(nodes.data(), heap, heap - 1)[0] == 0xABCD && g_path_calls == 4);
  // the smallest heaps: the root's children are a path of one
  CHECK(pc.find(2) != nullptr && pc.find(2)[0] == 16);  // (node 2 closes the path just fetched)
  pc.clear();
  CHECK(pc.get(nodes.data(), 4, 2)[0] == 16 && pc.levels == 1 && pc.get(nodes.data(), 4, 3)[0] == 24);
  CHECK(pc.get(nodes.data(), 8, 5)[0] == 40 && pc.levels == 2 && pc.find(3) != nullptr && pc.find(3)[7] == 31);
  // an error of the device call is thrown with its message, and the cache stays empty
  bool threw = false;
  try {
    pc.get(nodes.data(), 8, 9);
  } catch (const std::runtime_error& e) {
    threw = strstr(e.what(), "bad index") != nullptr;
  }
  CHECK(threw && pc.find(9) == nullptr && pc.find(5) == nullptr);
  // a moved cache keeps its path (Buf's move constructor)
  pc.get(nodes.data(), heap, heap - 2);
  PathCache moved(std::move(pc));
  CHECK(moved.find(heap - 2) != nullptr && moved.find(heap - 2)[0] == (heap - 2) * 8);
  printf("OK\n");
  return 0;
}
