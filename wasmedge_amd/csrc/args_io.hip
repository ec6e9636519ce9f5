// args_io.hip -- device-resident arguments and results (WasmEdge_BatchSetArgsDevice /
// ResultsDevice): rows of 64-bit slots in a caller's device buffer <-> the 32-bit cells the
// interpreter kernels read (KParams::params) and write (KParams::results). A translation unit
// of its own: the interpreter kernels' object does not change with it.
//
// Both sides are row-major, [n][stride] slots and [n][cells] cells, and a work item takes
// one element of the side it writes, so consecutive work items write consecutive words and
// read words at most a slot apart. Which word of the slot row a cell is (an i32 takes the low
// word of its slot, an i64 both, a v128 the four words of two slots) comes from a small
// per-signature table in device memory (args_io.h).
//
//   * wb_args_pack_kernel: a work item per (instance, cell); it also sums args_fp_mix over the
//     cells -- per wave with shuffles, per block through LDS, then one 64-bit atomic add per
//     block into a device word the host reads after the call's stream synchronise.
//   * wb_args_unpack_kernel: a work item per (instance, slot written); a block first loads the
//     status byte of each row it covers, once, and rows that did not end with 0 get zeroes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "args_io.h"

namespace {

constexpr uint32_t kMaxBlock = 1024;
constexpr uint32_t kMaxGrid = 2048;   // blocks; the rest by grid stride

// g = q * d + r (the 64-bit division only for an index past 2^32)
__device__ inline void split(uint64_t g, uint32_t d, uint32_t *q, uint32_t *r) {
  if (g <= 0xFFFFFFFFull) {
    *q = uint32_t(g) / d;
    *r = uint32_t(g) % d;
  } else {
    *q = uint32_t(g / d);
    *r = uint32_t(g % d);
  }
}

__global__ void __launch_bounds__(kMaxBlock) wb_args_pack_kernel(const ArgsPackParams p) {
  __shared__ uint64_t s_part[kMaxBlock / 64];
  const uint64_t total = uint64_t(p.n) * p.cells, step = uint64_t(gridDim.x) * blockDim.x;
  const uint32_t *words = reinterpret_cast<const uint32_t *>(p.slots);
  uint64_t acc = 0;
  for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < total; g += step) {
    uint32_t i, c;
    split(g, p.cells, &i, &c);
    const uint32_t v = words[uint64_t(i) * p.stride * 2u + p.word_of[c]];
    p.params[g] = v;
    acc += args_fp_mix(g, v);
  }
  for (uint32_t d = 32; d; d >>= 1) acc += __shfl_down(acc, d, 64);
  const uint32_t t = threadIdx.x;
  if ((t & 63u) == 0) s_part[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < (blockDim.x + 63u) >> 6; w++) acc += s_part[w];
    atomicAdd(reinterpret_cast<unsigned long long *>(p.fp), static_cast<unsigned long long>(acc));
  }
}

__global__ void __launch_bounds__(kMaxBlock) wb_args_unpack_kernel(const ArgsUnpackParams p) {
  __shared__ uint8_t s_status[kMaxBlock];
  const uint32_t per = p.words >> 1, t = threadIdx.x, bs = blockDim.x;
  const uint64_t total = uint64_t(p.n) * per, step = uint64_t(gridDim.x) * bs;
  // (base is uniform over the block: every thread takes every round and its barriers)
  for (uint64_t base = uint64_t(blockIdx.x) * bs; base < total; base += step) {
    // the block's elements [base, end] lie in rows [row0, row1], at most bs of them
    const uint64_t end = (base + bs < total ? base + bs : total) - 1u;
    uint32_t row0, r0, row1, r1;
    split(base, per, &row0, &r0);
    split(end, per, &row1, &r1);
    __syncthreads();   // (the previous round's readers of s_status)
    if (t <= row1 - row0) s_status[t] = p.status[row0 + t];
    __syncthreads();
    if (base + t > end) continue;
    const uint32_t k = r0 + t, i = row0 + k / per, s = k % per;   // (k < per + bs)
    uint64_t v = 0;
    if (s_status[i - row0] == 0) {
      const uint32_t *row = p.results + uint64_t(i) * p.cells;
      const uint32_t lo = p.cell_of[2u * s], hi = p.cell_of[2u * s + 1u];
      v = row[lo];
      if (hi != kArgsNoCell) v |= uint64_t(row[hi]) << 32;
    }
    p.slots[uint64_t(i) * p.stride + s] = v;
  }
}

uint32_t grid_for(uint64_t total, uint32_t block) {
  const uint64_t blocks = (total + block - 1u) / block;
  return uint32_t(blocks < kMaxGrid ? blocks : kMaxGrid);
}

}  // namespace

extern "C" uint32_t wb_args_io_block(void) {
  const char *e = getenv("WB_ARGS_BLOCK");
  const long b = e ? strtol(e, nullptr, 10) : 0;
  return b >= 64 && b <= long(kMaxBlock) && b % 64 == 0 ? uint32_t(b) : 256u;
}

extern "C" hipError_t wb_launch_args_pack(const ArgsPackParams *p, hipStream_t s) {
  const uint64_t total = uint64_t(p->n) * p->cells;
  if (!total) return hipSuccess;
  const uint32_t block = wb_args_io_block();
  hipLaunchKernelGGL(wb_args_pack_kernel, dim3(grid_for(total, block)), dim3(block), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t wb_launch_args_unpack(const ArgsUnpackParams *p, hipStream_t s) {
  const uint64_t total = uint64_t(p->n) * (p->words >> 1);
  if (!total) return hipSuccess;
  const uint32_t block = wb_args_io_block();
  hipLaunchKernelGGL(wb_args_unpack_kernel, dim3(grid_for(total, block)), dim3(block), 0, s, *p);
  return hipGetLastError();
}
