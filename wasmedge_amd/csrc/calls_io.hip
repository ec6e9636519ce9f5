// calls_io.hip -- device-resident per-instance calls (WasmEdge_BatchSetCallsDevice /
// CallsResultsDevice): a device vector FuncOf and rows of 64-bit slots in a caller's device
// buffer -> the call table and parameter cells the interpreter kernels read (KParams::calls,
// KParams::params), and KParams::results -> slot rows, each row by its own function's
// signature. A translation unit of its own: the interpreter kernels' object does not change
// with it.
//
// The signatures come from small tables in device memory (calls_io.h): one row per NAME for
// the pack kernel (FuncOf[i] indexes it), one row per MODULE FUNCTION for the unpack kernel
// (call_fn[i] indexes it). As in args_io.hip both sides are row-major and a work item takes
// one element of the side it writes, so consecutive work items write consecutive words.
//
//   * wb_calls_pack_kernel: a work item per (instance, cell) over the row stride pc; the item
//     of cell 0 also writes the instance's two call-table words and its function. It sums
//     args_fp_mix over the table words and the cells, takes the lowest instance whose FuncOf
//     names no function and notes whether a called function is an import -- per wave with
//     shuffles, per block through LDS, then at most three atomics per block into a 16-byte
//     summary the host reads after the call's stream synchronise.
//   * wb_calls_unpack_kernel: a work item per (instance, slot < width); a block first loads
//     the status byte and the function of each row it covers, once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "calls_io.h"
#include "kparams.h"

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

__global__ void __launch_bounds__(kMaxBlock) wb_calls_pack_kernel(const CallsPackParams p) {
  __shared__ uint64_t s_fp[kMaxBlock / 64];
  __shared__ uint32_t s_bad[kMaxBlock / 64], s_imp[kMaxBlock / 64];
  const uint64_t total = uint64_t(p.n) * p.pc, step = uint64_t(gridDim.x) * blockDim.x;
  const uint64_t cell0 = uint64_t(p.n) * 2u;   // the cells' fingerprint indices start here
  const uint32_t *words = reinterpret_cast<const uint32_t *>(p.slots);
  uint64_t acc = 0;
  uint32_t bad = 0, imp = 0;
  for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < total; g += step) {
    uint32_t i, c;
    split(g, p.pc, &i, &c);
    // (the consecutive items of a row read the same FuncOf word and table row)
    const uint32_t j = p.func_of[i];
    uint32_t entry = WB_CALL_SKIP, cells = 0, fn = 0xFFFFFFFFu, map = 0;
    if (j != kCallsNoCall) {
      if (j < p.nfuncs) {
        const uint32_t *f = p.table + size_t(j) * kCallsFnWords;
        entry = f[kCallsFnEntry];
        cells = f[kCallsFnCells];
        fn = f[kCallsFnFunc];
        map = f[kCallsFnMap];
        if (c == 0) imp |= f[kCallsFnImport];
      } else if (~i > bad) {
        bad = ~i;   // (the call fails; what this row gets is never run)
      }
    }
    uint32_t v = 0;
    if (c < cells) v = words[uint64_t(i) * p.stride * 2u + p.table[map + c]];
    p.params[g] = v;
    acc += args_fp_mix(cell0 + g, v);
    if (c == 0) {
      p.calls[2u * size_t(i)] = entry;
      p.calls[2u * size_t(i) + 1u] = cells;
      p.call_fn[i] = int32_t(fn);
      acc += args_fp_mix(2u * uint64_t(i), entry) + args_fp_mix(2u * uint64_t(i) + 1u, cells);
    }
  }
  for (uint32_t d = 32; d; d >>= 1) {
    acc += __shfl_down(acc, d, 64);
    const uint32_t b = __shfl_down(bad, d, 64);
    bad = b > bad ? b : bad;
    imp |= __shfl_down(imp, d, 64);
  }
  const uint32_t t = threadIdx.x;
  if ((t & 63u) == 0) {
    s_fp[t >> 6] = acc;
    s_bad[t >> 6] = bad;
    s_imp[t >> 6] = imp;
  }
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < (blockDim.x + 63u) >> 6; w++) {
      acc += s_fp[w];
      bad = s_bad[w] > bad ? s_bad[w] : bad;
      imp |= s_imp[w];
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(&p.sum->fp), static_cast<unsigned long long>(acc));
    if (bad) atomicMax(&p.sum->bad, bad);
    if (imp) atomicOr(&p.sum->imported, 1u);
  }
}

__global__ void __launch_bounds__(kMaxBlock) wb_calls_unpack_kernel(const CallsUnpackParams p) {
  __shared__ uint8_t s_status[kMaxBlock];
  __shared__ int32_t s_fn[kMaxBlock];
  // (width 0: one item per row still, for lens)
  const uint32_t per = p.width ? p.width : 1u, t = threadIdx.x, bs = blockDim.x;
  const uint64_t total = uint64_t(p.n) * per, step = uint64_t(gridDim.x) * bs;
  // (base is uniform over the block: every thread takes every round and its barriers)
  for (uint64_t base = uint64_t(blockIdx.x) * bs; base < total; base += step) {
    // the block's elements [base, end] lie in rows [row0, row1], at most bs of them
    const uint64_t end = (base + bs < total ? base + bs : total) - 1u;
    uint32_t row0, r0, row1, r1;
    split(base, per, &row0, &r0);
    split(end, per, &row1, &r1);
    __syncthreads();   // (the previous round's readers of s_status / s_fn)
    if (t <= row1 - row0) {
      s_status[t] = p.status[row0 + t];
      s_fn[t] = p.call_fn[row0 + t];
    }
    __syncthreads();
    if (base + t > end) continue;
    const uint32_t k = r0 + t, i = row0 + k / per, s = k % per;   // (k < per + bs)
    const int32_t fn = s_fn[i - row0];
    const uint32_t *f = fn >= 0 ? p.table + size_t(fn) * kCallsResWords : nullptr;
    if (s == 0 && p.lens) p.lens[i] = f ? f[kCallsResLen] : 0u;
    if (s >= p.width) continue;
    uint64_t v = 0;
    if (f && s_status[i - row0] == 0 && s < f[kCallsResSlots]) {
      const uint32_t *row = p.results + uint64_t(i) * p.cells;
      const uint32_t *m = p.table + f[kCallsResMap] + 2u * s;
      const uint32_t lo = m[0], hi = m[1];
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

extern "C" hipError_t wb_launch_calls_pack(const CallsPackParams *p, hipStream_t s) {
  const uint64_t total = uint64_t(p->n) * p->pc;
  if (!total) return hipSuccess;
  const uint32_t block = wb_args_io_block();
  hipLaunchKernelGGL(wb_calls_pack_kernel, dim3(grid_for(total, block)), dim3(block), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t wb_launch_calls_unpack(const CallsUnpackParams *p, hipStream_t s) {
  const uint64_t total = uint64_t(p->n) * (p->width ? p->width : 1u);
  if (!total) return hipSuccess;
  const uint32_t block = wb_args_io_block();
  hipLaunchKernelGGL(wb_calls_unpack_kernel, dim3(grid_for(total, block)), dim3(block), 0, s, *p);
  return hipGetLastError();
}
