// mem_spans.h -- launch parameters of the device-resident spans transfer (mem_spans.hip), by
// value. Plain C++ (no HIP types): the kernel bodies (mem_span_kernels.inc) also compile as
// host code, a thread per GPU thread, for a sanitizer rehearsal outside the library.
#pragma once
#include <stdint.h>

#include "mem_layout.h"

namespace wbp {

constexpr uint32_t kTileWords = 64;   // words of each lane in a tile / a piece (mem_io.hip kTile)

// A wave's class, decided by the plan kernel over the lanes that move bytes
enum WaveClass : uint32_t {
  kNone = 0,     // nobody moves
  kLane = 1,     // the per-lane body: own starts, any alignment
  kTile = 2,     // one 4-byte aligned start for all of them: the LDS tile, 4 bytes per thread
                 // on the rows' side
  kTile16 = 3,   // ... a 16-byte aligned start, Stride and buffer: 16 bytes per thread there too
};

constexpr uint32_t kOob = 0xFFFFFFFFu;     // a lane record's first word: out of bounds
constexpr uint32_t kNoBad = 0xFFFFFFFFu;   // summary[0]: no instance's length exceeds Len

// Blocks per wave of the move kernel, from Len alone: the words a range of Len bytes can touch
// (Len / 4 and one more at either end), from anywhere inside a first 64-word tile on.
WB_HOST_DEVICE inline uint32_t pieces_of(uint32_t len) {
  return uint32_t((uint64_t(len) / 4u + 2u + kTileWords - 2u) / kTileWords + 1u);
}

}  // namespace wbp

// Rows of a [n][stride] byte buffer <-> linear memory 0 of instances [0, n). Instance i moves
// len_i bytes between byte i * stride of `buf` and its memory at offset + off_i, where off_i /
// len_i are the low 32 bits of off_slots[i * off_stride] / len_slots[i * len_stride] (NULL: 0 /
// len). The plan kernel writes lane_plan, wave_plan and summary, which the context owns; the
// move kernel reads them and writes memory (or rows), status and the write marks.
struct MemSpanParams {
  uint32_t *mem;               // KParams::mem, the reserved layout
  uint32_t *lstate;            // KParams::lstate (LS_PAGES read; LS_HWM raised by a write)
  const uint64_t *ptab;        // KParams::ptab (or NULL: no pool rows)
  const uint64_t *off_slots;   // device, or NULL
  const uint64_t *len_slots;   // device, or NULL
  uint8_t *buf;                // device: the row of instance 0
  uint8_t *status;             // device [n] or NULL: 0 or MemoryOutOfBounds (0x88) per instance
  uint32_t *lane_plan;         // [nwaves * 64][2]: start byte (wbp::kOob: out of bounds), bytes
                               // to move (0: none)
  uint32_t *wave_plan;         // [nwaves][2]: wbp::WaveClass, the wave's start word (tile classes)
  uint32_t *summary;           // [4]: the lowest i with len_i > len (from wbp::kNoBad, atomic min),
                               // instances out of bounds, waves of a tile class, 0
  uint32_t *next_summary;      // [4]: the next call's summary, which this plan sets to its
                               // starting values {wbp::kNoBad, 0, 0, 0}
  uint64_t off_stride, len_stride, stride;
  uint32_t mem_words, mlog, ptab_w, ls_slots;
  uint32_t n, nwaves;
  uint32_t offset, len;
  uint32_t align;              // the host's finding on buf and stride: 16, 4 or 1
  uint32_t pieces;             // wbp::pieces_of(len)
  uint32_t write;              // 1: buf -> memory, 0: memory -> buf
};

#if defined(__HIPCC__)
// p->summary holds {wbp::kNoBad, 0, 0, 0}: the previous plan's next_summary, or the caller's copy
extern "C" hipError_t wb_launch_span_plan(const MemSpanParams *p, hipStream_t s);
extern "C" hipError_t wb_launch_span_move(const MemSpanParams *p, hipStream_t s);
#endif
