// mem_layout.h -- where a word of linear memory sits in a wave's lane-interleaved region:
// one definition for the host views (batch_ctx.h, hostcall.cpp) and for device code that
// addresses memory from outside the interpreter (mem_io.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WB_HOST_DEVICE __host__ __device__
#else
#define WB_HOST_DEVICE
#endif

namespace wbh {

// Word `w` of lane `lane` within its wave's memory region, granules of 2^g words
// (dbc_ops.h GMem): ((w >> g) * 64 + lane) * 2^g + (w & (2^g - 1)).
WB_HOST_DEVICE inline size_t lane_word(uint64_t w, uint32_t lane, uint32_t g) {
  return (size_t(w >> g) << (6 + g)) + (size_t(lane) << g) + size_t(w & ((1u << g) - 1u));
}

}  // namespace wbh
