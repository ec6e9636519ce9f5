// mem_io.hip -- bulk linear-memory transfer (WasmEdge_BatchWriteMemories / ReadMemories):
// rows of a row-major [instances][stride] byte buffer <-> memory 0 of every instance, the
// batched form of WasmEdge_MemoryInstanceSetData / GetData (wasmedge.h:2552-2569). A
// translation unit of its own: the interpreter kernels' object does not change with it.
//
// Memory is lane-interleaved per wave in granules of 2^g words (mem_layout.h lane_word), pages
// past the reserved layout in pool rows behind the page table (kparams.h "Paged linear
// memory"), so the transfer is a transposing gather / scatter. Each lane checks its own range
// against its size (LS_PAGES), as the reference's bound check does (memory.h:74-78): a lane
// past it gets MemoryOutOfBounds and moves nothing; a write raises the lane's write mark
// (LS_HWM), as WaveView::rw does, so that the next Reset restores what it wrote.
//
// Two kernels, both over plain vector loads and stores:
//   * wb_mem_io_tile_kernel: no per-instance offsets, everything 4-byte aligned. A block
//     moves a tile of 64 lanes x 64 words through LDS. The tile is aligned in memory, where
//     it is one contiguous 16 KiB piece of the wave's region (64 words is a multiple of every
//     granule), moved 16 bytes per thread: a wave's access is 1 KiB contiguous, which lane
//     and word a piece holds following from g as wb_mem_hash_kernel's comment sets out. On
//     the buffer's side a wave moves 256 contiguous bytes of a row (4 bytes per thread), or
//     of 4 rows (16 bytes per thread, ROW16: offset, stride and buffer 16-byte aligned).
//     Rows of the LDS tile are 65 words apart: a column access (one word of 64 lanes) and a
//     row access both spread over the banks. Only whole words go through the tile; a lane
//     whose length is not a multiple of 4 merges its last 1..3 bytes on its own.
//   * wb_mem_io_lane_kernel: the general path. A thread takes one word of one lane at a
//     time: the lane's own offset and alignment, a first and last word merged byte by byte
//     (they belong to that lane alone), any granule, page or pool-row crossing. Lanes with
//     the same offset still touch adjacent words of memory; the buffer's side is a gather.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"
#include "mem_io.h"
#include "mem_layout.h"

using wbh::lane_word;

namespace {

typedef uint32_t wb_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kTile = 64;           // words of each lane in a tile / a chunk
constexpr uint32_t kPitch = kTile + 1;   // LDS row pitch (words): breaks the power-of-2 stride
constexpr uint8_t kOutOfBounds = 0x88;   // ErrCode::MemoryOutOfBounds

// Lane `lane` of wave `wave`: its range [start, start + len), len 0 when it moves nothing
// (not in [first, last), out of bounds, or an empty range). `report`: one block per wave
// also writes the lane's status byte and raises its write mark.
__device__ inline void lane_span(const MemIoParams &p, uint32_t wave, uint32_t lane, bool report,
                                 uint32_t *start, uint32_t *len) {
  *start = *len = 0;
  const uint32_t inst = wave * 64u + lane;
  if (inst < p.first || inst >= p.last) return;
  uint32_t l = p.lens ? p.lens[inst] : p.len;
  if (l > p.len) l = p.len;   // (the host refuses such a call; nothing here depends on it)
  const uint64_t s = (uint64_t)p.offset + (p.offsets ? p.offsets[inst] : 0u), e = s + l;
  const uint32_t pages = p.lstate[((size_t)wave * p.ls_slots + LS_PAGES) * 64u + lane];
  const bool ok = e <= ((uint64_t)pages << 16);   // memory.h:74-78
  if (report) {
    p.status[inst] = ok ? 0 : kOutOfBounds;
    if (p.write && ok && l) {
      uint32_t *mark = &p.lstate[((size_t)wave * p.ls_slots + LS_HWM) * 64u + lane];
      if (e > *mark) *mark = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
    }
  }
  if (ok && l) {   // (then s < 2^32)
    *start = (uint32_t)s;
    *len = l;
  }
}

// The wave's region that holds word `w` of its lanes -- the reserved layout, or the pool row
// of w's page -- and w's index within it (*wl, for lane_word); nullptr: no such row.
__device__ inline uint32_t *region(const MemIoParams &p, uint32_t wave, uint32_t w, uint32_t *wl) {
  const uint32_t page = w >> 14, rp = p.mem_words >> 14;
  if (page < rp) {
    *wl = w;
    return p.mem + (size_t)wave * p.mem_words * 64u;
  }
  const uint32_t k = page - rp;
  if (!p.ptab || k >= p.ptab_w) return nullptr;
  *wl = w & 16383u;
  return (uint32_t *)(uintptr_t)p.ptab[(size_t)wave * p.ptab_w + k];
}

__device__ inline uint8_t *row_of(const MemIoParams &p, uint32_t inst) {
  return p.buf + (uint64_t)(inst - p.first) * p.stride;
}

// bytes [0, nb) of `bytes` <-> bytes [sh/8, sh/8 + nb) of the memory word at `word`
template <bool WRITE>
__device__ inline void merge_bytes(uint32_t *word, uint8_t *bytes, uint32_t sh, uint32_t nb) {
  uint32_t v = *word;
  for (uint32_t q = 0; q < 4; q++) {
    if (q >= nb) break;
    const uint32_t s = sh + 8u * q;
    if (WRITE) v = (v & ~(0xFFu << s)) | ((uint32_t)bytes[q] << s);
    else bytes[q] = (uint8_t)(v >> s);
  }
  if (WRITE) *word = v;
}

// ---- the general path --------------------------------------------------------------------
// Block (wave, c): word k = c * 64 + j of every lane's range, counted from the lane's own
// first word; thread t serves lane t & 63, words j = (t >> 6) + 4 * (0..15).
template <bool WRITE>
__global__ void __launch_bounds__(256) wb_mem_io_lane_kernel(const MemIoParams p, uint32_t chunks) {
  __shared__ uint32_t s_start[64], s_len[64];
  const uint32_t t = threadIdx.x, lane = t & 63u, w0 = p.first >> 6;
  const uint64_t total = (uint64_t)(((p.last + 63u) >> 6) - w0) * chunks;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const uint32_t wave = w0 + (uint32_t)(b / chunks), c = (uint32_t)(b % chunks);
    __syncthreads();   // (the previous round's readers of s_*)
    if (t < 64) lane_span(p, wave, t, c == 0, &s_start[t], &s_len[t]);
    __syncthreads();
    const uint32_t len = s_len[lane];
    if (!len) continue;
    const uint64_t start = s_start[lane], end = start + len;
    const uint32_t fw = (uint32_t)(start >> 2), nwords = (uint32_t)((end + 3u) >> 2) - fw;
    uint8_t *row = row_of(p, wave * 64u + lane);
    for (uint32_t j = 0; j < kTile / 4u; j++) {
      const uint32_t k = c * kTile + (t >> 6) + 4u * j;
      if (k >= nwords) break;
      const uint32_t w = fw + k;
      uint32_t wl;
      uint32_t *reg = region(p, wave, w, &wl);
      if (!reg) continue;
      uint32_t *word = reg + lane_word(wl, lane, p.mlog);
      const uint64_t wb = (uint64_t)w << 2;
      const uint64_t lo = start > wb ? start : wb, hi = end < wb + 4u ? end : wb + 4u;
      uint8_t *bytes = row + (lo - start);
      if (hi - lo == 4u && ((uintptr_t)bytes & 3u) == 0) {
        if (WRITE) *word = *(const uint32_t *)bytes;
        else *(uint32_t *)bytes = *word;
      } else {
        merge_bytes<WRITE>(word, bytes, 8u * (uint32_t)(lo & 3u), (uint32_t)(hi - lo));
      }
    }
  }
}

// ---- the tiled path ----------------------------------------------------------------------
// Block (wave, tile): words [W0, W0 + 64) of the wave's 64 lanes, W0 = tb + 64 * tile a
// multiple of 64; word w of a lane is word w - sw of its row (sw = offset / 4).
template <bool WRITE, bool ROW16>
__global__ void __launch_bounds__(256) wb_mem_io_tile_kernel(const MemIoParams p, uint32_t tiles) {
  __shared__ uint32_t tile[64 * kPitch];
  __shared__ uint32_t s_len[64];
  const uint32_t t = threadIdx.x, g = p.mlog, gm = (1u << g) - 1u, w0 = p.first >> 6;
  const uint32_t sw = p.offset >> 2, tb = sw & ~(kTile - 1u);
  const uint64_t total = (uint64_t)(((p.last + 63u) >> 6) - w0) * tiles;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const uint32_t wave = w0 + (uint32_t)(b / tiles), ti = (uint32_t)(b % tiles);
    const uint32_t W0 = tb + ti * kTile;
    __syncthreads();   // (the previous round's readers of tile / s_len)
    if (t < 64) {
      uint32_t start;
      lane_span(p, wave, t, ti == 0, &start, &s_len[t]);
    }
    __syncthreads();
    uint32_t wl0;
    uint32_t *reg = region(p, wave, W0, &wl0);   // (uniform over the block)
    if (!reg) continue;
    // word W0 + wi of `lane` goes through the tile: a whole word of its range
#define WB_IN_TILE(lane, wi) (W0 + (wi) >= sw && W0 + (wi) - sw < (s_len[lane] >> 2))
    // memory side: piece x / 4 of the tile's 16 KiB, elements x .. x + 3; element x is word
    // (x >> (6 + g) << g) + (x & gm) of lane (x >> g) & 63, at lane_word() of the two
#define WB_MEM_SIDE(BODY)                                                                    \
    for (uint32_t k = 0; k < 4; k++) {                                                       \
      const uint32_t x = 4u * (t + 256u * k);                                                \
      uint32_t ln[4], wi[4];                                                                 \
      bool in[4];                                                                            \
      for (uint32_t q = 0; q < 4; q++) {                                                     \
        ln[q] = ((x + q) >> g) & 63u;                                                        \
        wi[q] = (((x + q) >> (6u + g)) << g) + ((x + q) & gm);                               \
        in[q] = WB_IN_TILE(ln[q], wi[q]);                                                    \
      }                                                                                      \
      uint32_t *at = reg + lane_word(wl0 + wi[0], ln[0], g);   /* = tile region + x */       \
      BODY                                                                                   \
    }
    // buffer side: ROW16: words 4 * (t & 15) .. + 3 of rows (t >> 4) + 16 * (0..3);
    // else word t & 63 of rows (t >> 6) + 4 * (0..15)
#define WB_ROW_SIDE(BODY16, BODY4)                                                           \
    if (ROW16) {                                                                             \
      for (uint32_t k = 0; k < 4; k++) {                                                     \
        const uint32_t lane = (t >> 4) + 16u * k, wi = 4u * (t & 15u);                       \
        bool in[4];                                                                          \
        for (uint32_t q = 0; q < 4; q++) in[q] = WB_IN_TILE(lane, wi + q);                   \
        if (!(in[0] || in[1] || in[2] || in[3])) continue;                                   \
        uint32_t *at = (uint32_t *)row_of(p, wave * 64u + lane) + ((int64_t)W0 + wi - sw);   \
        uint32_t *cell = &tile[lane * kPitch + wi];                                          \
        BODY16                                                                               \
      }                                                                                      \
    } else {                                                                                 \
      for (uint32_t k = 0; k < 16; k++) {                                                    \
        const uint32_t lane = (t >> 6) + 4u * k, wi = t & 63u;                               \
        if (!WB_IN_TILE(lane, wi)) continue;                                                 \
        uint32_t *at = (uint32_t *)row_of(p, wave * 64u + lane) + ((int64_t)W0 + wi - sw);   \
        uint32_t *cell = &tile[lane * kPitch + wi];                                          \
        BODY4                                                                                \
      }                                                                                      \
    }
    if (WRITE) {
      WB_ROW_SIDE(
          if (in[0] && in[1] && in[2] && in[3]) {
            const wb_u32x4 v = *(const wb_u32x4 *)at;
            cell[0] = v.x; cell[1] = v.y; cell[2] = v.z; cell[3] = v.w;
          } else {
            for (uint32_t q = 0; q < 4; q++)
              if (in[q]) cell[q] = at[q];
          },
          *cell = *at;)
      __syncthreads();
      WB_MEM_SIDE(
          if (in[0] && in[1] && in[2] && in[3]) {
            wb_u32x4 v;
            v.x = tile[ln[0] * kPitch + wi[0]]; v.y = tile[ln[1] * kPitch + wi[1]];
            v.z = tile[ln[2] * kPitch + wi[2]]; v.w = tile[ln[3] * kPitch + wi[3]];
            *(wb_u32x4 *)at = v;
          } else {
            for (uint32_t q = 0; q < 4; q++)
              if (in[q]) at[q] = tile[ln[q] * kPitch + wi[q]];
          })
    } else {
      WB_MEM_SIDE(
          if (in[0] || in[1] || in[2] || in[3]) {   // (the whole piece lies in the region)
            const wb_u32x4 v = *(const wb_u32x4 *)at;
            tile[ln[0] * kPitch + wi[0]] = v.x; tile[ln[1] * kPitch + wi[1]] = v.y;
            tile[ln[2] * kPitch + wi[2]] = v.z; tile[ln[3] * kPitch + wi[3]] = v.w;
          })
      __syncthreads();
      WB_ROW_SIDE(
          if (in[0] && in[1] && in[2] && in[3]) {
            wb_u32x4 v;
            v.x = cell[0]; v.y = cell[1]; v.z = cell[2]; v.w = cell[3];
            *(wb_u32x4 *)at = v;
          } else {
            for (uint32_t q = 0; q < 4; q++)
              if (in[q]) at[q] = cell[q];
          },
          *at = *cell;)
    }
    // a lane's last 1..3 bytes: its own word, past the words the tile moved
    if (t < 64 && (s_len[t] & 3u)) {
      const uint32_t w = sw + (s_len[t] >> 2);
      if (w >= W0 && w < W0 + kTile)
        merge_bytes<WRITE>(reg + lane_word(wl0 + (w - W0), t, g),
                           row_of(p, wave * 64u + t) + (s_len[t] & ~3u), 0, s_len[t] & 3u);
    }
#undef WB_ROW_SIDE
#undef WB_MEM_SIDE
#undef WB_IN_TILE
  }
}

bool aligned(const MemIoParams *p, uint32_t a) {
  return p->offset % a == 0 && p->stride % a == 0 && (uintptr_t)p->buf % a == 0;
}

}  // namespace

extern "C" int wb_mem_io_tiled(const MemIoParams *p) { return !p->offsets && aligned(p, 4); }

extern "C" hipError_t wb_launch_mem_io(const MemIoParams *p, hipStream_t s) {
  if (p->last <= p->first) return hipSuccess;
  const uint64_t waves = ((p->last + 63u) >> 6) - (p->first >> 6);
  // words a lane's range can touch: len / 4, and one more at either end when unaligned
  const uint64_t end_word = ((uint64_t)p->offset + p->len + 3u) >> 2;
  uint64_t per_wave;
  const bool tiled = wb_mem_io_tiled(p);
  if (tiled) {
    const uint64_t tb = (p->offset >> 2) & ~(uint64_t)(kTile - 1u);
    per_wave = (end_word - tb + kTile - 1u) / kTile;
  } else {
    per_wave = ((uint64_t)p->len / 4u + 2u + kTile - 1u) / kTile;
  }
  if (per_wave == 0) per_wave = 1;   // (the status bytes)
  const uint64_t total = waves * per_wave;
  const dim3 grid((uint32_t)(total < (1u << 20) ? total : (1u << 20))), block(256);
  const uint32_t pw = (uint32_t)per_wave;
  if (!tiled) {
    if (p->write) hipLaunchKernelGGL(wb_mem_io_lane_kernel<true>, grid, block, 0, s, *p, pw);
    else hipLaunchKernelGGL(wb_mem_io_lane_kernel<false>, grid, block, 0, s, *p, pw);
  } else if (aligned(p, 16)) {
    if (p->write) hipLaunchKernelGGL((wb_mem_io_tile_kernel<true, true>), grid, block, 0, s, *p, pw);
    else hipLaunchKernelGGL((wb_mem_io_tile_kernel<false, true>), grid, block, 0, s, *p, pw);
  } else {
    if (p->write) hipLaunchKernelGGL((wb_mem_io_tile_kernel<true, false>), grid, block, 0, s, *p, pw);
    else hipLaunchKernelGGL((wb_mem_io_tile_kernel<false, false>), grid, block, 0, s, *p, pw);
  }
  return hipGetLastError();
}
