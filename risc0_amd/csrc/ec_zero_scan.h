// The zero scan of eval_check's gate columns, restated for the host: which of n columns of
// `words` words hold no nonzero word. zero_scan (eltwise.hip) answers the same on the device,
// where a wave ORs its words, ballots, and sets the column's bit in the "seen nonzero" flags with
// at most one atomic; the mask handed back is the complement of those flags over the n columns.
// No HIP header: the generated kernels' host translation unit (tools/gen_eval_check.py --host)
// and the CPU tests compile this.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "evalcheck_types.h"

namespace r0 {

// the mask handed back: the n columns whose "seen nonzero" bit is clear
inline uint64_t zero_scan_dead(uint64_t seen, int n) {
  const uint64_t all = n >= kMaxGates ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
  return ~seen & all;
}

// bit g of the result: column g is zero in all `words` words
inline uint64_t zero_scan_host(const uint32_t* const* cols, int n, size_t words) {
  uint64_t seen = 0;
  for (int g = 0; g < n && g < kMaxGates; g++) {
    uint32_t v = 0;
    for (size_t i = 0; i < words; i++) v |= cols[g][i];
    if (v) seen |= uint64_t(1) << g;
  }
  return zero_scan_dead(seen, n);
}

}  // namespace r0
