// snapshot_plan.h -- the planning of instance snapshots that does not touch the device
// (snapshot.cpp; DESIGN.md "Instance snapshots"). Host-only and free of HIP, so that a
// stand-alone host program can share it with the library: how many rows of a wave a
// snapshot holds, where they sit in the packed buffer, which source every destination lane
// draws from, the class of every destination wave and the tiles a restore visits.
#pragma once
#include <stdint.h>

#include <vector>

#include "snapshot.h"

namespace wbs {

// a source-map entry of a selective restore (WASMEDGE_BATCH_SNAPSHOT_KEEP): the lane keeps
// what it holds
constexpr uint32_t kKeep = 0xFFFFFFFFu;

// (rows_of_mark, the rows of a wave that can differ from zero given its highest write mark:
// snapshot.h, shared with the kernels)

inline uint32_t wave_mark(const uint32_t *marks64) {
  uint32_t m = 0;
  for (uint32_t l = 0; l < 64; l++) m = marks64[l] > m ? marks64[l] : m;
  return m;
}

// marks: [nwaves][64] write marks (LS_HWM). rows[w] = the rows wave w's snapshot holds,
// off[w] = the first word of its rows in the packed buffer (rows[w] * 64 words, wave after
// wave); returns the buffer's words.
inline uint64_t pack_rows(const uint32_t *marks, uint32_t nwaves, uint32_t image_words, uint32_t mem_words,
                          std::vector<uint32_t> *rows, std::vector<uint64_t> *off) {
  rows->assign(nwaves, 0);
  off->assign(nwaves, 0);
  uint64_t total = 0;
  for (uint32_t w = 0; w < nwaves; w++) {
    (*rows)[w] = rows_of_mark(wave_mark(marks + size_t(w) * 64), image_words, mem_words);
    (*off)[w] = total;
    total += uint64_t((*rows)[w]) * 64u;
  }
  return total;
}

// The captured instance that lane `inst` (of nwaves * 64, the last wave's lanes past n
// included) restarts from. A lane past n never runs; it follows lane 0 of its wave into that
// lane's source wave, keeping its own lane number, so that it does not turn a broadcast or a
// permutation within a wave into a gather. kKeep (a selective restore: the lane keeps what it
// holds) is carried through, and a lane past n is kept when lane 0 of its wave is.
inline uint32_t source_of(const uint32_t *src_of, uint32_t n, uint32_t inst) {
  if (!src_of) return inst;
  if (inst < n) return src_of[inst];
  const uint32_t s0 = src_of[inst & ~63u];
  return s0 == kKeep ? kKeep : (s0 & ~63u) | (inst & 63u);
}

enum WaveClass : uint32_t {
  kIdentity = 0,   // every lane from itself, same granule: tiles are copied as they lie
  kOneWave = 1,    // every lane from one source wave: its tile is read whole, permuted in LDS
  kGather = 2,     // lanes from several waves: every lane gathers its source lane's words
  kKeepAll = 3,    // every lane kept (selective restore): the wave is not visited
};
// beside the class of a wave that restores some lanes and keeps others: its class is that of
// its restored lanes alone, and the memory-0 restore writes it lane by lane (gather kernel)
constexpr uint32_t kHasKeep = 0x100u, kClassMask = 0xFFu;

struct RestorePlan {
  std::vector<uint32_t> src;    // [nwaves * 64] source_of every lane (kKeep carried through)
  std::vector<uint32_t> wave;   // [nwaves][2]: WaveClass (| kHasKeep), tiles the sources of its
                                // restored lanes hold (the largest)
  uint32_t max_tiles = 0;       // the largest of those
  bool identity = true;         // no wave needs the gather kernel: each is kIdentity without a
                                // kept lane, or kKeepAll
  bool any_keep = false;        // some lane (below n) is kept
  uint32_t restored = 0;        // instances (below n) that are not kept
};

// snap_rows: [nwaves] rows each captured wave holds (multiples of kTile). Every src_of[i]
// must be below n or kKeep (the caller checked).
inline void plan_restore(const uint32_t *src_of, uint32_t n, uint32_t nwaves, const uint32_t *snap_rows,
                         bool same_granule, RestorePlan *P) {
  P->src.resize(size_t(nwaves) * 64);
  P->wave.assign(size_t(nwaves) * 2, 0);
  P->max_tiles = 0;
  P->identity = true;
  P->any_keep = false;
  P->restored = 0;
  for (uint32_t w = 0; w < nwaves; w++) {
    bool self = same_granule, one = true;
    uint32_t tiles = 0, kept = 0, first = kKeep;   // first: the source of the first restored lane
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t i = w * 64 + l, s = source_of(src_of, n, i);
      P->src[i] = s;
      if (s == kKeep) {
        kept++;
        P->any_keep = P->any_keep || i < n;
        continue;
      }
      if (i < n) P->restored++;
      if (first == kKeep) first = s;
      self = self && s == i;
      one = one && (s >> 6) == (first >> 6);
      const uint32_t t = snap_rows[s >> 6] / kTile;
      tiles = t > tiles ? t : tiles;
    }
    const uint32_t cls = kept == 64 ? kKeepAll : (self ? kIdentity : one ? kOneWave : kGather) | (kept ? kHasKeep : 0u);
    P->wave[2 * size_t(w)] = cls;
    P->wave[2 * size_t(w) + 1] = tiles;
    P->max_tiles = tiles > P->max_tiles ? tiles : P->max_tiles;
    P->identity = P->identity && (cls == kIdentity || cls == kKeepAll);
  }
}

// ---- the call stack of a suspended invocation (DESIGN.md "Snapshots of suspended runs") -----
// A lane parked with LS_GSP = g owns HBM rows [0, g - gs_lds) of its wave's call stack
// (batch_kernel.hip GS_RD / GS_WR: slots below gs_lds are LDS, saved with the frame), and
// nothing above them is ever read. rpc, gsp: [nwaves][64] LS_RPC / LS_GSP. S_w = the largest
// max(0, gsp - gs_lds) over the wave's parked lanes (rpc != ~0, instance below n), rounded up
// to a tile, within the gs_depth rows allocated.
inline uint32_t stack_rows(const uint32_t *rpc64, const uint32_t *gsp64, uint32_t lanes, uint32_t gs_lds,
                           uint32_t gs_depth) {
  uint64_t s = 0;
  for (uint32_t l = 0; l < lanes && l < 64; l++)
    if (rpc64[l] != 0xFFFFFFFFu && gsp64[l] > gs_lds && gsp64[l] - gs_lds > s) s = gsp64[l] - gs_lds;
  s = (s + kTile - 1u) & ~uint64_t(kTile - 1u);
  return uint32_t(s < gs_depth ? s : gs_depth);
}

// rows[w] = S_w, off[w] = the first word of wave w's rows in the packed buffer (rows[w] * 64
// words, wave after wave); returns the buffer's words.
inline uint64_t pack_stack(const uint32_t *rpc, const uint32_t *gsp, uint32_t n, uint32_t nwaves, uint32_t gs_lds,
                           uint32_t gs_depth, std::vector<uint32_t> *rows, std::vector<uint64_t> *off) {
  rows->assign(nwaves, 0);
  off->assign(nwaves, 0);
  uint64_t total = 0;
  for (uint32_t w = 0; w < nwaves; w++) {
    const uint32_t lanes = n > w * 64u ? (n - w * 64u < 64u ? n - w * 64u : 64u) : 0u;
    (*rows)[w] = stack_rows(rpc + size_t(w) * 64, gsp + size_t(w) * 64, lanes, gs_lds, gs_depth);
    (*off)[w] = total;
    total += uint64_t((*rows)[w]) * 64u;
  }
  return total;
}

// The restore of those rows. src: [nwaves * 64] the source of every lane (RestorePlan::src) or
// NULL: every lane from itself. wave: [nwaves][2] -- the class (kIdentity: the wave's own rows
// copied as they lie; else every lane gathers its source lane's word of a row: at the stack's
// 4-byte granule one source wave or several make the same loads, the rows of one wave merely
// share cache lines) and the rows its sources hold (the largest: rows of a lane above its own
// source's are never read and get zero). Returns the largest of those: the depth the
// context's stack needs.
inline uint32_t plan_stack(const uint32_t *src, uint32_t nwaves, const uint32_t *stack_rows_of,
                           std::vector<uint32_t> *wave) {
  wave->assign(size_t(nwaves) * 2, 0);
  uint32_t need = 0;
  for (uint32_t w = 0; w < nwaves; w++) {
    bool self = true, one = true;
    uint32_t rows = 0;
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t i = w * 64 + l, s = src ? src[i] : i;
      self = self && s == i;
      one = one && (s >> 6) == ((src ? src[size_t(w) * 64] : i) >> 6);
      const uint32_t r = (s >> 6) < nwaves ? stack_rows_of[s >> 6] : 0u;
      rows = r > rows ? r : rows;
    }
    (*wave)[2 * size_t(w)] = self ? kIdentity : one ? kOneWave : kGather;
    (*wave)[2 * size_t(w) + 1] = rows;
    need = rows > need ? rows : need;
  }
  return need;
}

// Tiles a restore visits for a destination wave: up to the larger of what its sources hold
// (copied, or image / zero for a lane whose own source wave holds less) and the wave's
// current bound `cur_rows` (rows_of_mark of its marks now: re-initialised).
inline uint32_t visit_tiles(uint32_t src_tiles, uint32_t cur_rows) {
  const uint32_t cur = cur_rows / kTile;
  return src_tiles > cur ? src_tiles : cur;
}

}  // namespace wbs
