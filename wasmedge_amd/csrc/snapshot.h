// snapshot.h -- launch parameters of the instance-snapshot kernels (snapshot.hip), by value.
// Plain C++ (no HIP types): the kernel bodies (snapshot_kernels.inc) also compile as host
// code, a thread per GPU thread, for a sanitizer rehearsal outside the library.
#pragma once
#include <stdint.h>

#include "mem_layout.h"

namespace wbs {

constexpr uint32_t kTile = 64;   // words of each lane in a tile: 16 KiB of a wave, contiguous
                                 // at every granule (64 words is a multiple of each)

// Rows (words per lane) of a wave's reserved layout that can differ from zero: Reset's bound
// (batch_kernel.hip wb_mem_init_kernel) -- max(ceil(highest write mark / 4), image_words),
// within mem_words -- rounded up to a tile. mem_words is a multiple of 16384 (or 0).
WB_HOST_DEVICE inline uint32_t rows_of_mark(uint32_t mark_bytes, uint32_t image_words, uint32_t mem_words) {
  const uint64_t hw = (uint64_t(mark_bytes) + 3u) / 4u;
  uint64_t rows = hw < mem_words ? hw : mem_words;
  if (rows < image_words && image_words <= mem_words) rows = image_words;
  rows = (rows + kTile - 1u) & ~uint64_t(kTile - 1u);
  return uint32_t(rows < mem_words ? rows : mem_words);
}

}  // namespace wbs

// Memory 0. A snapshot holds rows [0, snap_rows[w]) of every wave w, lane-interleaved at the
// granule it was taken under, packed wave after wave: wave w's rows start at word snap_off[w]
// of `snap`. Every loop bound below comes from these host-made tables or from the wave's
// write marks clamped to mem_words.
struct SnapMemParams {
  uint32_t *mem;               // the context's reserved layout (KParams::mem)
  uint32_t *snap;              // the packed rows
  const uint64_t *snap_off;    // [nwaves]
  const uint32_t *snap_rows;   // [nwaves] multiples of 64, <= mem_words
  const uint32_t *lstate;      // KParams::lstate: the waves' current marks (restore)
  const uint32_t *image;       // the module image (image_words words)
  const uint32_t *src;         // [nwaves * 64] source instance of every lane, or wbs::kKeep (gather)
  const uint32_t *wave_plan;   // [nwaves][2]: wbs::WaveClass (| wbs::kHasKeep), tiles the sources
                               // of its restored lanes hold (gather; a copy that keeps lanes
                               // reads it for wbs::kKeepAll alone)
  uint32_t nwaves, mem_words, ls_slots, image_words;
  uint32_t g_mem, g_snap;      // log2 words per granule: the layout's now, the snapshot's
  uint32_t chunks;             // blocks per wave; block (w, c) takes tiles c, c + chunks, ...
};

// The HBM part of the call stack (KParams::gstack, [wave][gs_depth][64] at the 4-byte granule)
// of a suspended invocation. A snapshot holds rows [0, snap_rows[w]) of wave w -- the rows its
// parked lanes own -- packed as memory 0's: wave w's rows start at word snap_off[w] of `snap`
// (snap_words words). The kernels clamp every row count to gs_depth and to the packed buffer.
struct SnapStackParams {
  uint32_t *gstack;            // the context's call stack
  uint32_t *snap;              // the packed rows
  const uint64_t *snap_off;    // [nwaves] multiples of 64
  const uint32_t *snap_rows;   // [nwaves]
  const uint32_t *src;         // [nwaves * 64] source instance of every lane (fork)
  const uint32_t *wave_plan;   // [nwaves][2]: wbs::WaveClass, rows its sources hold (fork)
  uint64_t snap_words;
  uint32_t nwaves, gs_depth;   // gs_depth: rows of a wave in `gstack` now
  uint32_t chunks;             // blocks per wave; block (w, c) takes 16-byte pieces c * 256 + t, ...
};

// The arrays indexed by instance (status, counts, hcall, the result rows): instance i from
// instance src_of[i].
struct SnapInstParams {
  uint8_t *status_d;
  const uint8_t *status_s;
  uint64_t *counts_d;
  const uint64_t *counts_s;
  uint32_t *hcall_d;
  const uint32_t *hcall_s;
  uint32_t *results_d;
  const uint32_t *results_s;   // [n][result_cells] both
  const uint32_t *src_of;      // [>= n] or NULL: every instance from itself
  uint32_t n, result_cells;
};

// Whole-buffer state (instance-state slots, per-lane tables, memories 1..7, their sizes):
// word base_d + k (k < count) of lane l of wave w, in a [wave][words][64] buffer interleaved
// in granules of 2^g words, from the same word (at base_s) of its source lane -- or `fill`
// when src is NULL. g > 0 needs base_d, base_s and count multiples of 2^g. A lane whose src_of
// entry is wbs::kKeep (keep != 0: a selective restore) is left as it is, fill included.
struct SnapRowsParams {
  uint32_t *dst;
  const uint32_t *src;         // or NULL: fill
  const uint32_t *src_of;      // [nwaves * 64] or NULL: every lane from itself
  uint32_t nwaves, words_d, words_s, base_d, base_s, count, g, fill;
  uint32_t ls_fix;             // 1: instance state -- LS_RPC / LS_GSP / LS_HBASE "not parked", kept
                               // lanes included (0 for a snapshot that holds the invocation:
                               // kept as captured)
  uint32_t keep;               // 1: src_of may hold wbs::kKeep (wb_snap_select_rows_kernel)
};

// The plan of a selective restore from a source map on the device (wb_snap_plan_kernel): what
// wbs::plan_restore makes on the host, written where the host's plan is uploaded.
struct SnapPlanParams {
  const uint32_t *map;         // [n] the caller's: a source instance or wbs::kKeep
  const uint32_t *snap_rows;   // [nwaves] (SnapMemParams)
  uint32_t *plan_src;          // [nwaves * 64] out: RestorePlan::src
  uint32_t *wave_plan;         // [nwaves][2] out: RestorePlan::wave
  uint32_t *summary;           // [4], zeroed by the caller: ~(the lowest invalid i) or 0, any lane
                               // kept, any wave for the gather kernel, instances restored
  uint32_t n, nwaves, same_granule;
};
