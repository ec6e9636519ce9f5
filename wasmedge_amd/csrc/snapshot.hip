// snapshot.hip -- instance snapshots on the device (WasmEdge_BatchSnapshotCreate / Restore;
// DESIGN.md "Instance snapshots"). A translation unit of its own, like mem_io.hip: the
// interpreter kernels' object does not change with it.
//
// Memory 0 lives lane-interleaved per wave in granules of 2^g words (mem_layout.h), and only
// the rows below a wave's write-mark bound can differ from zero (wb_mem_init_kernel's
// invariant), so a snapshot holds those rows alone, packed wave after wave:
//   * wb_snap_capture_kernel: the rows of every wave into the packed buffer;
//   * wb_snap_restore_copy_kernel: every lane from itself under the capture's granule -- a
//     streaming copy of the held tiles, then the tail up to the wave's current bound
//     re-initialised from the image / zero;
//   * wb_snap_restore_gather_kernel: lanes from other lanes (fork) or under another granule,
//     a tile at a time through LDS;
//   * wb_snap_rows_kernel: the small whole buffers (instance state, per-lane tables, memories
//     1..7 and their sizes) through the same source map.
// A selective restore (DESIGN.md "Selective restore") leaves the lanes its map keeps as they
// are. It launches kernels of its own -- wb_snap_select_copy / _gather / _rows_kernel, the same
// bodies instantiated with the kept-lane paths --, so that a restore without kept lanes runs
// the kernels it always ran, and adds
//   * wb_snap_plan_kernel: the plan of a restore from a source map that lives on the device.
// A snapshot that holds a suspended invocation (DESIGN.md "Snapshots of suspended runs") adds
//   * wb_snap_stack_capture_kernel / wb_snap_stack_copy_kernel: the HBM rows of the call stack
//     that a wave's parked lanes own, packed the same way, out and back as they lie;
//   * wb_snap_stack_fork_kernel: those rows through the source map, a word gather per lane;
//   * wb_snap_inst_kernel: status, count, hcall and result row of every instance from its
//     source's (the frame-save rows go through wb_snap_rows_kernel).
// The bodies are in snapshot_kernels.inc, which also compiles as host code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"
#include "mem_layout.h"
#include "snapshot.h"
#include "snapshot_plan.h"

#define WB_SNAP_FN __device__ inline
#define WB_SNAP_SYNC() __syncthreads()
#define WB_SNAP_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define WB_SNAP_ATOMIC_OR(p, v) atomicOr((p), (v))
#define WB_SNAP_ATOMIC_ADD(p, v) atomicAdd((p), (v))

namespace {

#include "snapshot_kernels.inc"

__global__ void __launch_bounds__(256) wb_snap_capture_kernel(const SnapMemParams p) {
  snap_capture_body(p, blockIdx.x, threadIdx.x);
}

__global__ void __launch_bounds__(256) wb_snap_restore_copy_kernel(const SnapMemParams p) {
  __shared__ uint32_t s_m[64];
  snap_restore_copy_body<false>(p, blockIdx.x, threadIdx.x, s_m);
}

__global__ void __launch_bounds__(256) wb_snap_select_copy_kernel(const SnapMemParams p) {
  __shared__ uint32_t s_m[64];
  snap_restore_copy_body<true>(p, blockIdx.x, threadIdx.x, s_m);
}

__global__ void __launch_bounds__(256) wb_snap_restore_gather_kernel(const SnapMemParams p) {
  __shared__ uint32_t tile[64 * kSnapPitch];
  __shared__ uint32_t s_m[64], s_src[64];
  snap_restore_gather_body(p, blockIdx.x, threadIdx.x, tile, s_m, s_src);
}

__global__ void __launch_bounds__(256) wb_snap_select_gather_kernel(const SnapMemParams p) {
  __shared__ uint32_t tile[64 * kSnapPitch];
  __shared__ uint32_t s_m[64], s_src[64], s_keep[64];
  snap_select_gather_body(p, blockIdx.x, threadIdx.x, tile, s_m, s_src, s_keep);
}

__global__ void __launch_bounds__(256) wb_snap_rows_kernel(const SnapRowsParams p) {
  snap_rows_body<false>(p, (size_t)blockIdx.x * 256u + threadIdx.x, (size_t)gridDim.x * 256u);
}

__global__ void __launch_bounds__(256) wb_snap_select_rows_kernel(const SnapRowsParams p) {
  snap_rows_body<true>(p, (size_t)blockIdx.x * 256u + threadIdx.x, (size_t)gridDim.x * 256u);
}

// the plan of a selective restore from a source map on the device: a block per wave
__global__ void __launch_bounds__(64) wb_snap_plan_kernel(const SnapPlanParams p) {
  __shared__ uint32_t s_src[64], s_tiles[64], s_bad[64];
  snap_plan_body(p, blockIdx.x, threadIdx.x, s_src, s_tiles, s_bad);
}

// a suspended invocation (DESIGN.md "Snapshots of suspended runs"): the HBM rows of the call
// stack that parked lanes own, and the arrays indexed by instance
__global__ void __launch_bounds__(256) wb_snap_stack_capture_kernel(const SnapStackParams p) {
  snap_stack_copy_body(p, blockIdx.x, threadIdx.x, false);
}

__global__ void __launch_bounds__(256) wb_snap_stack_copy_kernel(const SnapStackParams p) {
  snap_stack_copy_body(p, blockIdx.x, threadIdx.x, true);
}

__global__ void __launch_bounds__(256) wb_snap_stack_fork_kernel(const SnapStackParams p) {
  snap_stack_fork_body(p, blockIdx.x, threadIdx.x);
}

__global__ void __launch_bounds__(256) wb_snap_inst_kernel(const SnapInstParams p) {
  snap_inst_body(p, (size_t)blockIdx.x * 256u + threadIdx.x, (size_t)gridDim.x * 256u);
}

}  // namespace

// kind 0: capture, 1: restore (every wave from itself), 2: restore (through p->src)
extern "C" hipError_t wb_launch_snap_stack(const SnapStackParams *p, int kind, hipStream_t s) {
  if (p->nwaves == 0 || p->gs_depth == 0 || p->chunks == 0 || p->snap_words == 0) return hipSuccess;
  const dim3 grid(p->nwaves * p->chunks), block(256);
  if (kind == 0) hipLaunchKernelGGL(wb_snap_stack_capture_kernel, grid, block, 0, s, *p);
  else if (kind == 1) hipLaunchKernelGGL(wb_snap_stack_copy_kernel, grid, block, 0, s, *p);
  else hipLaunchKernelGGL(wb_snap_stack_fork_kernel, grid, block, 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t wb_launch_snap_inst(const SnapInstParams *p, hipStream_t s) {
  if (p->n == 0) return hipSuccess;
  hipLaunchKernelGGL(wb_snap_inst_kernel, dim3((p->n + 255u) / 256u), dim3(256), 0, s, *p);
  return hipGetLastError();
}

// kind 0: capture, 1: restore (copy), 2: restore (gather), 3 / 4: the same for a restore that
// keeps lanes (the wave plan is read by both); p->chunks blocks per wave
extern "C" hipError_t wb_launch_snap_mem(const SnapMemParams *p, int kind, hipStream_t s) {
  if (p->nwaves == 0 || p->mem_words == 0 || p->chunks == 0) return hipSuccess;
  const dim3 grid(p->nwaves * p->chunks), block(256);
  if (kind == 0) hipLaunchKernelGGL(wb_snap_capture_kernel, grid, block, 0, s, *p);
  else if (kind == 1) hipLaunchKernelGGL(wb_snap_restore_copy_kernel, grid, block, 0, s, *p);
  else if (kind == 2) hipLaunchKernelGGL(wb_snap_restore_gather_kernel, grid, block, 0, s, *p);
  else if (kind == 3) hipLaunchKernelGGL(wb_snap_select_copy_kernel, grid, block, 0, s, *p);
  else hipLaunchKernelGGL(wb_snap_select_gather_kernel, grid, block, 0, s, *p);
  return hipGetLastError();
}

// the caller zeroed p->summary on the same stream
extern "C" hipError_t wb_launch_snap_plan(const SnapPlanParams *p, hipStream_t s) {
  if (p->nwaves == 0) return hipSuccess;
  hipLaunchKernelGGL(wb_snap_plan_kernel, dim3(p->nwaves), dim3(64), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t wb_launch_snap_rows(const SnapRowsParams *p, hipStream_t s) {
  const uint64_t total = (uint64_t)p->nwaves * p->count * 64u;
  if (total == 0) return hipSuccess;
  const uint64_t blocks = (total + 1023u) / 1024u;   // (4 words per thread where it is large)
  const dim3 grid((uint32_t)(blocks < 65536u ? blocks : 65536u));
  if (p->keep) hipLaunchKernelGGL(wb_snap_select_rows_kernel, grid, dim3(256), 0, s, *p);
  else hipLaunchKernelGGL(wb_snap_rows_kernel, grid, dim3(256), 0, s, *p);
  return hipGetLastError();
}
