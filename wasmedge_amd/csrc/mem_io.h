// mem_io.h -- launch parameters of the bulk linear-memory transfer (mem_io.hip), by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Rows of a [last - first][stride] byte buffer <-> linear memory 0 of instances
// [first, last): instance i moves min(lens[i], len) bytes (lens NULL: len) between byte
// (i - first) * stride of `buf` and its memory at offset + offsets[i] (offsets NULL: 0).
struct MemIoParams {
  uint32_t *mem;             // KParams::mem, the reserved layout
  uint32_t *lstate;          // KParams::lstate (LS_PAGES read; LS_HWM raised by a write)
  const uint64_t *ptab;      // KParams::ptab (or NULL: no pool rows)
  const uint32_t *offsets;   // device, [n] (indexed by instance) or NULL
  const uint32_t *lens;      // device, [n] or NULL
  uint8_t *buf;              // device: the row of instance `first`
  uint8_t *status;           // device, [n]: 0 or MemoryOutOfBounds (0x88) per instance
  uint64_t stride;
  uint32_t mem_words, mlog, rpages, ptab_w, ls_slots;
  uint32_t first, last;      // last <= NumInstances
  uint32_t offset, len;
  uint32_t write;            // 1: buf -> memory, 0: memory -> buf
};

// 1 when the launch takes the tiled path (wb_launch_mem_io picks it; DESIGN.md "Bulk memory
// transfer"), else the per-lane general path
extern "C" int wb_mem_io_tiled(const MemIoParams *p);
extern "C" hipError_t wb_launch_mem_io(const MemIoParams *p, hipStream_t s);
