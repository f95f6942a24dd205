// Device buffers for the host driver: pooled allocations (the bench proves the
// same shapes back to back, so blocks are recycled by exact size instead of
// paying hipMalloc/hipFree per segment) and a small RAII owner.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace r0 {

void* dev_alloc(size_t bytes);
void dev_free(void* p);
void dev_trim();  // return pooled blocks to the driver
// An allocation of its own (a recursion program handle's buffers): never a block of a thread's
// pool or scratch, so no thread's release hands it on and any stream may read it. Counted in
// MemStats (live and reserved) from the call to dev_free_dedicated, which returns it to the driver.
void* dev_alloc_dedicated(size_t bytes);
void dev_free_dedicated(void* p, size_t bytes);
// page-locked host buffers (r0hip_host_alloc): freed blocks are kept pinned for reuse,
// host_trim() returns the idle ones to the driver
void* host_alloc(size_t bytes);
void host_free(void* p);
void host_trim();
void set_device(int ordinal);

// RAII buffer of u32 words. A borrowed DevBuf (DevBuf::borrow) names words someone else owns,
// read-only for whoever holds it: it frees nothing, moved or destroyed.
struct DevBuf {
  uint32_t* p = nullptr;
  size_t words = 0;
  bool owned = true;
  DevBuf() = default;
  explicit DevBuf(size_t w) : p(static_cast<uint32_t*>(dev_alloc(w * 4))), words(w) {}
  static DevBuf borrow(const uint32_t* q, size_t w) {
    DevBuf b;
    b.p = const_cast<uint32_t*>(q);
    b.words = w;
    b.owned = false;
    return b;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), words(o.words), owned(o.owned) {
    o.p = nullptr;
    o.words = 0;
    o.owned = true;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (owned) dev_free(p);
      p = o.p;
      words = o.words;
      owned = o.owned;
      o.p = nullptr;
      o.words = 0;
      o.owned = true;
    }
    return *this;
  }
  ~DevBuf() {
    if (owned) dev_free(p);
  }
};

// The device half of a register group's commitment (prover.cpp, commit_group_device):
// coefficients, evaluations and the whole Merkle node heap, queued on some stream; nothing read
// back yet.
struct GroupWork {
  DevBuf coeffs, evaluated, nodes;
  size_t count = 0;
};

// A register group committed once and kept (a recursion program handle's control group): the
// three buffers of a GroupWork, complete, owned by the handle and read-only, with the host copy
// of the tree's root and top layers that MerkleTree::finish would read back (node 1 .. the end
// of the top layer, 8 words each).
struct CachedGroup {
  const uint32_t *coeffs, *evaluated, *nodes;
  size_t count;
  const uint32_t* top;
};

}  // namespace r0
