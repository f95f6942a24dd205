// The injector in its compact form (include/r0hip.h, r0hip_backs): the host side shared by the
// per-op call, r0hip_prove_segment_trace_backs and the worker (api.cpp). The expansion itself is
// rv32im_inject_backs (rv32im_witgen.hip).
#pragma once
#include <string>
#include <vector>

#include "../../include/r0hip.h"

namespace r0 {

static_assert(sizeof(r0hip_back) == 12, "r0hip_back is three words (rv32im_inject_backs reads it so)");

// What the host check counts on its way: the (offset, value) pairs the records expand to (the
// set_cycle columns not included) and the BigInt records.
struct BacksInfo {
  size_t entries = 0;
  size_t n_bigint = 0;
};
// The host check of a caller's r0hip_backs against a segment of seg_rows rows, O(n records), before
// any launch: null arrays with a nonzero count, inj_rows <= seg_rows, rows strictly increasing and
// below inj_rows, kinds 1..4, payloads inside `words`. Throws "<who>: ..." naming the record.
BacksInfo check_backs(const r0hip_backs* b, size_t seg_rows, const std::string& who);
// The accumulation's records (r0hip_bigint_back: row, poly_op, coeff, bytes) from the BigInt
// payloads of checked backs (BigIntState::as_array: words 3, 4 and 5..20), in record order.
std::vector<r0hip_bigint_back> backs_bigint_records(const r0hip_backs& b, size_t n_bigint);

// prove_trace's injector when it comes as Back records: the arrays (device pointers if the trace
// is resident, else the caller's checked host arrays) and the check's counts.
struct TraceBacks {
  const uint32_t* recs;
  size_t n;
  const uint32_t* words;
  size_t n_words;
  size_t inj_rows;
  size_t entries;
};

}  // namespace r0
