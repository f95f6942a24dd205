// The device interpreter of a run-time circuit's constraint program (eval_interp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "circuit_rt.h"

namespace r0 {

// The slot file of one launch stays under this many bytes: half the 256 MiB Infinity Cache, so a
// chunk's slots are re-read from cache and not from HBM.
constexpr size_t kInterpSlotBudget = size_t(128) << 20;

// What the kernels read of the programs, as one word array for dev_table: the records, the
// eval_check tap table, the rows tap table, the extension constants.
std::vector<uint32_t> interp_device_image(const rt::Programs& p);
// Points per launch for n points: the budget's choice (a multiple of the workgroup, at least
// one), or the calling thread's r0hip_testing_set_interp_chunk value; never above n.
uint32_t interp_chunk_points(const rt::Programs& p, size_t n);
uint32_t set_interp_test_chunk(uint32_t points) noexcept;  // returns the previous value
// Queue the program over n points on s, `lanes` points per launch. d_slots: lanes *
// p.slot_words() words. rows: the constraint_rows form (d_acc written), else the eval_check form
// (d_check written, d_vinv read). d_args: device table of the eval_check argument buffers.
void eval_interp(hipStream_t s, bool rows, const rt::Programs& p, const uint32_t* d_image,
                 const uint32_t* const* d_args, const uint32_t* d_pow, size_t n, uint32_t* d_slots, uint32_t lanes,
                 const uint32_t* d_vinv, uint32_t* d_check, uint32_t* d_acc);

}  // namespace r0
