// mem_spans.hip -- device-resident spans (WasmEdge_BatchWriteMemoriesSpansDevice /
// ReadMemoriesSpansDevice; DESIGN.md "Device-resident spans"): the bulk linear-memory transfer
// of mem_io.hip with every instance's offset and length read from 64-bit slots on the device,
// a column of a BatchResultsDevice buffer as it lies. A translation unit of its own: the
// objects of the interpreter kernels and of mem_io.hip do not change with it.
//
//   * wb_span_plan_kernel: a wave of 64 threads per wave of instances. A lane reads its two
//     slots and its size and decides in range / out of bounds; ballots over the lanes that
//     will move bytes class the wave: one shared, 4-byte aligned start -> the tile body
//     (16-byte rows where start, Stride and buffer allow), else the per-lane body. It writes the
//     lane records, the wave's class and start word and a summary of a few words, all owned by
//     the context: nothing the caller can see. The host reads the summary back before it
//     launches the move, so that a length past Len leaves everything untouched.
//   * wb_span_move_kernel: one launch over (wave, piece), the pieces per wave from Len alone.
//     A block reads its wave's class -- a block-uniform branch -- and runs the tile body or
//     the per-lane body of mem_io.hip; the block of a wave's first piece writes the status
//     bytes (when asked for) and raises the write marks.
// The bodies are in mem_span_kernels.inc, which also compiles as host code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"
#include "mem_layout.h"
#include "mem_spans.h"

#define WB_SPAN_FN __device__ inline
#define WB_SPAN_SYNC() __syncthreads()
#define WB_SPAN_BALLOT(pred, t) ((uint64_t)__ballot(pred))
#define WB_SPAN_BCAST(v, lane, t) ((uint32_t)__shfl((int)(v), (int)(lane)))
#define WB_SPAN_ATOMIC_MIN(p, v) atomicMin((p), (v))
#define WB_SPAN_ATOMIC_ADD(p, v) atomicAdd((p), (v))

namespace {

#include "mem_span_kernels.inc"

__global__ void __launch_bounds__(64) wb_span_plan_kernel(const MemSpanParams p) {
  if (blockIdx.x < p.nwaves) span_plan_body(p, blockIdx.x, threadIdx.x);
}

template <bool WRITE>
__global__ void __launch_bounds__(256) wb_span_move_kernel(const MemSpanParams p) {
  __shared__ uint32_t tile[64 * kSpanPitch];
  __shared__ uint32_t s_start[64], s_len[64];
  const uint64_t total = (uint64_t)p.nwaves * p.pieces;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    __syncthreads();   // (the previous round's readers of tile / s_*)
    span_move_body<WRITE>(p, b, threadIdx.x, tile, s_start, s_len);
  }
}

}  // namespace

extern "C" hipError_t wb_launch_span_plan(const MemSpanParams *p, hipStream_t s) {
  if (p->nwaves == 0) return hipSuccess;
  hipLaunchKernelGGL(wb_span_plan_kernel, dim3(p->nwaves), dim3(64), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t wb_launch_span_move(const MemSpanParams *p, hipStream_t s) {
  const uint64_t total = (uint64_t)p->nwaves * p->pieces;
  if (total == 0) return hipSuccess;
  const dim3 grid((uint32_t)(total < (1u << 20) ? total : (1u << 20))), block(256);
  if (p->write) hipLaunchKernelGGL(wb_span_move_kernel<true>, grid, block, 0, s, *p);
  else hipLaunchKernelGGL(wb_span_move_kernel<false>, grid, block, 0, s, *p);
  return hipGetLastError();
}
