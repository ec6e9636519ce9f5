// snapshot_kernels.inc -- the bodies of the instance-snapshot kernels (snapshot.hip wraps each
// in a __global__ function). Plain loads and stores only. The including file defines
//   WB_SNAP_FN      the function qualifiers (__device__ inline; host: inline)
//   WB_SNAP_SYNC()  the block barrier (__syncthreads(); host: a barrier of 256 threads)
// so that the same text runs as host code, a thread per GPU thread, under a sanitizer.
// A block has 256 threads; block b serves wave b / chunks and, of that wave's tiles,
// c = b % chunks, c + chunks, ... A tile is 64 words of the wave's 64 lanes: 16 KiB, one
// contiguous piece of the wave's region at every granule, moved 16 bytes per thread (a wave's
// access: 1 KiB contiguous). Element x of a tile's 4096 words under granules of 2^g words is
// word ((x >> (6 + g)) << g) + (x & (2^g - 1)) of lane (x >> g) & 63 (mem_io.hip).
// The call-stack bodies (at the end) take the same (wave, chunk) blocks over 16-byte pieces
// of a wave's rows; the bodies over whole buffers and over instances take a flat thread index.

typedef uint32_t wb_snap_v4 __attribute__((vector_size(16)));

constexpr uint32_t kSnapPitch = wbs::kTile + 1u;   // LDS row pitch, as mem_io.hip's tile

WB_SNAP_FN uint32_t snap_elem_lane(uint32_t x, uint32_t g) { return (x >> g) & 63u; }
WB_SNAP_FN uint32_t snap_elem_word(uint32_t x, uint32_t g) {
  return ((x >> (6u + g)) << g) + (x & ((1u << g) - 1u));
}

// the wave's current bound (rows), from its 64 write marks; s_m: 64 words of LDS
WB_SNAP_FN uint32_t snap_cur_rows(const SnapMemParams &p, uint32_t wave, uint32_t t, uint32_t *s_m) {
  if (t < 64) s_m[t] = p.lstate[((size_t)wave * p.ls_slots + LS_HWM) * 64u + t];
  WB_SNAP_SYNC();
  uint32_t m = 0;
  for (uint32_t l = 0; l < 64; l++) m = s_m[l] > m ? s_m[l] : m;
  return wbs::rows_of_mark(m, p.image_words, p.mem_words);   // (clamped to mem_words)
}

// tile ti of the wave at `to`: the module image, zero past it
WB_SNAP_FN void snap_init_tile(const SnapMemParams &p, uint32_t *to, uint32_t ti, uint32_t t) {
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t x = 4u * (t + 256u * k);
    wb_snap_v4 v;
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t w = ti * wbs::kTile + snap_elem_word(x + q, p.g_mem);
      v[q] = w < p.image_words ? p.image[w] : 0u;
    }
    *(wb_snap_v4 *)(to + x) = v;
  }
}

// ---- capture: rows [0, snap_rows[wave]) of the layout -> the packed buffer ------------------
WB_SNAP_FN void snap_capture_body(const SnapMemParams &p, uint32_t b, uint32_t t) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  const uint32_t rows = p.snap_rows[wave] < p.mem_words ? p.snap_rows[wave] : p.mem_words;
  const wb_snap_v4 *from = (const wb_snap_v4 *)(p.mem + (size_t)wave * p.mem_words * 64u);
  wb_snap_v4 *to = (wb_snap_v4 *)(p.snap + p.snap_off[wave]);
  for (uint32_t ti = c; ti < rows / wbs::kTile; ti += p.chunks)
    for (uint32_t k = 0; k < 4; k++) {
      const size_t i = (size_t)ti * 1024u + t + 256u * k;
      to[i] = from[i];
    }
}

// ---- restore, identity: every lane from itself, under the granule of the capture ----------
// Tiles below the snapshot's rows are copied as they lie; tiles from there up to the wave's
// current bound are re-initialised (Reset's work on the tail). SELECT (a restore that keeps
// lanes, a kernel of its own): a wave whose lanes are all kept is not visited.
template <bool SELECT>
WB_SNAP_FN void snap_restore_copy_body(const SnapMemParams &p, uint32_t b, uint32_t t, uint32_t *s_m) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  if (SELECT && p.wave_plan[2u * wave] == wbs::kKeepAll) return;
  const uint32_t cur = snap_cur_rows(p, wave, t, s_m) / wbs::kTile;
  const uint32_t rows = p.snap_rows[wave] < p.mem_words ? p.snap_rows[wave] : p.mem_words;
  const uint32_t held = rows / wbs::kTile, ntiles = held > cur ? held : cur;
  uint32_t *wm = p.mem + (size_t)wave * p.mem_words * 64u;
  const wb_snap_v4 *from = (const wb_snap_v4 *)(p.snap + p.snap_off[wave]);
  for (uint32_t ti = c; ti < ntiles; ti += p.chunks) {
    if (ti >= held) {
      snap_init_tile(p, wm + (size_t)ti * 4096u, ti, t);
      continue;
    }
    wb_snap_v4 *to = (wb_snap_v4 *)wm;
    for (uint32_t k = 0; k < 4; k++) {
      const size_t i = (size_t)ti * 1024u + t + 256u * k;
      to[i] = from[i];
    }
  }
}

// ---- restore, gather: lanes from other lanes, or under another granule ---------------------
// tile: 64 * kSnapPitch words of LDS; s_m, s_src: 64 words each. The destination side is
// always written 16 bytes per thread, contiguous. wbs::kOneWave: the one source wave's tile
// is read contiguously into LDS rows by SOURCE lane and every destination lane reads its
// source's row. wbs::kGather: 4 threads per destination lane read its source lane's 64 words
// -- pieces of 4 << g_snap bytes, 16 bytes per load where the granule holds them, single
// words at the 4-byte granule -- into LDS rows by DESTINATION lane. A lane whose source wave
// holds no rows of the tile gets the image / zero.
WB_SNAP_FN void snap_restore_gather_body(const SnapMemParams &p, uint32_t b, uint32_t t, uint32_t *tile,
                                         uint32_t *s_m, uint32_t *s_src) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  const uint32_t cur = snap_cur_rows(p, wave, t, s_m) / wbs::kTile;
  if (t < 64) {
    const uint32_t s = p.src[(size_t)wave * 64u + t];
    s_src[t] = (s >> 6) < p.nwaves ? s : wave * 64u + t;   // (the host's plan: always in range)
  }
  WB_SNAP_SYNC();
  const uint32_t cls = p.wave_plan[2u * wave], cap = p.mem_words / wbs::kTile;
  const uint32_t held = p.wave_plan[2u * wave + 1u] < cap ? p.wave_plan[2u * wave + 1u] : cap;
  const uint32_t ntiles = held > cur ? held : cur;
  const uint32_t gd = p.g_mem, gs = p.g_snap;
  uint32_t *wm = p.mem + (size_t)wave * p.mem_words * 64u;
  for (uint32_t ti = c; ti < ntiles; ti += p.chunks) {
    uint32_t *to = wm + (size_t)ti * 4096u;
    const bool one = cls != wbs::kGather;
    if (one) {
      const uint32_t sw = s_src[0] >> 6;
      const uint32_t rows = p.snap_rows[sw] < p.mem_words ? p.snap_rows[sw] : p.mem_words;
      if (ti >= rows / wbs::kTile) {   // (uniform over the block)
        snap_init_tile(p, to, ti, t);
        continue;
      }
      WB_SNAP_SYNC();   // (the previous round's readers of tile)
      const uint32_t *from = p.snap + p.snap_off[sw] + (size_t)ti * 4096u;
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t x = 4u * (t + 256u * k);
        const wb_snap_v4 v = *(const wb_snap_v4 *)(from + x);
        for (uint32_t q = 0; q < 4; q++)
          tile[snap_elem_lane(x + q, gs) * kSnapPitch + snap_elem_word(x + q, gs)] = v[q];
      }
    } else {
      WB_SNAP_SYNC();
      const uint32_t l = t >> 2, s = s_src[l], sw = s >> 6, sl = s & 63u;
      const uint32_t rows = p.snap_rows[sw] < p.mem_words ? p.snap_rows[sw] : p.mem_words;
      const bool in = ti < rows / wbs::kTile;
      const uint32_t *from = p.snap + p.snap_off[sw];
      for (uint32_t j = 0; j < 4; j++) {
        const uint32_t k = 4u * ((t & 3u) + 4u * j), w = ti * wbs::kTile + k;
        uint32_t *cell = &tile[l * kSnapPitch + k];
        if (!in) {
          for (uint32_t q = 0; q < 4; q++) cell[q] = w + q < p.image_words ? p.image[w + q] : 0u;
        } else if (gs >= 2) {   // (4 words of a granule: contiguous and 16-byte aligned)
          const wb_snap_v4 v = *(const wb_snap_v4 *)(from + wbh::lane_word(w, sl, gs));
          for (uint32_t q = 0; q < 4; q++) cell[q] = v[q];
        } else {
          for (uint32_t q = 0; q < 4; q++) cell[q] = from[wbh::lane_word(w + q, sl, gs)];
        }
      }
    }
    WB_SNAP_SYNC();
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t x = 4u * (t + 256u * k);
      wb_snap_v4 v;
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t ln = snap_elem_lane(x + q, gd);
        v[q] = tile[(one ? (s_src[ln] & 63u) : ln) * kSnapPitch + snap_elem_word(x + q, gd)];
      }
      *(wb_snap_v4 *)(to + x) = v;
    }
  }
}

// ---- restore that keeps lanes (DESIGN.md "Selective restore"), a kernel of its own ---------
// The gather above with kept lanes: s_keep is 64 more words of LDS. A wave of class
// wbs::kKeepAll is not visited. In a wave flagged wbs::kHasKeep the LDS tile is filled for the
// restored lanes as above (s_keep[l]: 1 for a kept lane; the one source wave is that of the first
// restored lane) and the write-out selects word by word: a thread first loads the 16 bytes it
// is about to store -- the live tile, contiguous like the store -- and puts back a kept lane's
// words as they were; where a granule holds the four words (g_mem >= 2) they are one lane's,
// and a kept lane's piece is neither loaded nor stored. A tile no source holds takes the same
// path with the image / zero for the restored lanes.
// MIXED is a template parameter: the wrapper below read the wave's plan (cls, tiles) and chose
// per wave, so a wave without kept lanes pays for no kept-lane test inside the loops. (A
// restore without kept lanes does not come here at all: it launches the gather above.)
template <bool MIXED>
WB_SNAP_FN void snap_select_gather_wave(const SnapMemParams &p, uint32_t wave, uint32_t c, uint32_t cls,
                                        uint32_t tiles, uint32_t t, uint32_t *tile, uint32_t *s_m,
                                        uint32_t *s_src, uint32_t *s_keep) {
  constexpr bool mixed = MIXED;
  const uint32_t cur = snap_cur_rows(p, wave, t, s_m) / wbs::kTile;
  if (t < 64) {
    const uint32_t s = p.src[(size_t)wave * 64u + t];
    if (mixed) s_keep[t] = s == wbs::kKeep ? 1u : 0u;
    s_src[t] = (s >> 6) < p.nwaves ? s : wave * 64u + t;   // (the plan: in range, or kept)
  }
  WB_SNAP_SYNC();
  uint32_t first = 0;   // the first restored lane (a mixed wave has one)
  if (mixed)
    while (first < 63u && s_keep[first]) first++;
  const uint32_t cap = p.mem_words / wbs::kTile;
  const uint32_t held = tiles < cap ? tiles : cap;
  const uint32_t ntiles = held > cur ? held : cur;
  const uint32_t gd = p.g_mem, gs = p.g_snap;
  uint32_t *wm = p.mem + (size_t)wave * p.mem_words * 64u;
  for (uint32_t ti = c; ti < ntiles; ti += p.chunks) {
    uint32_t *to = wm + (size_t)ti * 4096u;
    const bool one = cls != wbs::kGather;
    bool init = false;   // mixed, one source wave: it holds no rows of the tile
    if (one) {
      const uint32_t sw = s_src[first] >> 6;
      const uint32_t rows = p.snap_rows[sw] < p.mem_words ? p.snap_rows[sw] : p.mem_words;
      init = ti >= rows / wbs::kTile;   // (uniform over the block)
      if (init && !mixed) {
        snap_init_tile(p, to, ti, t);
        continue;
      }
    }
    if (MIXED && init) {
      // (nothing to stage: the write-out below takes the image / zero)
    } else if (one) {
      const uint32_t sw = s_src[first] >> 6;
      WB_SNAP_SYNC();   // (the previous round's readers of tile)
      const uint32_t *from = p.snap + p.snap_off[sw] + (size_t)ti * 4096u;
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t x = 4u * (t + 256u * k);
        const wb_snap_v4 v = *(const wb_snap_v4 *)(from + x);
        for (uint32_t q = 0; q < 4; q++)
          tile[snap_elem_lane(x + q, gs) * kSnapPitch + snap_elem_word(x + q, gs)] = v[q];
      }
    } else {
      WB_SNAP_SYNC();
      const uint32_t l = t >> 2, s = s_src[l], sw = s >> 6, sl = s & 63u;
      const uint32_t rows = p.snap_rows[sw] < p.mem_words ? p.snap_rows[sw] : p.mem_words;
      const bool in = ti < rows / wbs::kTile;
      const uint32_t *from = p.snap + p.snap_off[sw];
      for (uint32_t j = 0; j < 4 && !(mixed && s_keep[l]); j++) {
        const uint32_t k = 4u * ((t & 3u) + 4u * j), w = ti * wbs::kTile + k;
        uint32_t *cell = &tile[l * kSnapPitch + k];
        if (!in) {
          for (uint32_t q = 0; q < 4; q++) cell[q] = w + q < p.image_words ? p.image[w + q] : 0u;
        } else if (gs >= 2) {   // (4 words of a granule: contiguous and 16-byte aligned)
          const wb_snap_v4 v = *(const wb_snap_v4 *)(from + wbh::lane_word(w, sl, gs));
          for (uint32_t q = 0; q < 4; q++) cell[q] = v[q];
        } else {
          for (uint32_t q = 0; q < 4; q++) cell[q] = from[wbh::lane_word(w + q, sl, gs)];
        }
      }
    }
    WB_SNAP_SYNC();
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t x = 4u * (t + 256u * k);
      if (mixed && gd >= 2 && s_keep[snap_elem_lane(x, gd)]) continue;   // (one kept lane's piece)
      wb_snap_v4 v, live = {0u, 0u, 0u, 0u};
      if (mixed && gd < 2) live = *(const wb_snap_v4 *)(to + x);
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t ln = snap_elem_lane(x + q, gd), w = snap_elem_word(x + q, gd);
        if (mixed && s_keep[ln]) v[q] = live[q];
        else if (MIXED && init) v[q] = ti * wbs::kTile + w < p.image_words ? p.image[ti * wbs::kTile + w] : 0u;
        else v[q] = tile[(one ? (s_src[ln] & 63u) : ln) * kSnapPitch + w];
      }
      *(wb_snap_v4 *)(to + x) = v;
    }
  }
}

WB_SNAP_FN void snap_select_gather_body(const SnapMemParams &p, uint32_t b, uint32_t t, uint32_t *tile,
                                        uint32_t *s_m, uint32_t *s_src, uint32_t *s_keep) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  // (both words of the wave's plan with one load, before the first barrier)
  const uint32_t plan = p.wave_plan[2u * wave], tiles = p.wave_plan[2u * wave + 1u], cls = plan & wbs::kClassMask;
  if (cls == wbs::kKeepAll) return;
  if (plan & wbs::kHasKeep) snap_select_gather_wave<true>(p, wave, c, cls, tiles, t, tile, s_m, s_src, s_keep);
  else snap_select_gather_wave<false>(p, wave, c, cls, tiles, t, tile, s_m, s_src, s_keep);
}

// ---- whole-buffer state through the source map ----------------------------------------------
// thread i of `stride` threads; the destination side is contiguous, the source side a gather
// of single words (these buffers are small beside memory 0). KEEP (a restore that keeps
// lanes, a kernel of its own): a lane whose src_of entry is wbs::kKeep is left as it is.
template <bool KEEP>
WB_SNAP_FN void snap_rows_body(const SnapRowsParams &p, size_t i, size_t stride) {
  const size_t per = (size_t)p.count * 64u, total = per * p.nwaves;
  const uint32_t g = p.g;
  for (size_t x = i; x < total; x += stride) {
    const uint32_t w = (uint32_t)(x / per);
    const size_t r = x % per;
    const uint32_t l = (uint32_t)(r >> g) & 63u;
    const size_t k = ((r >> (6u + g)) << g) + (r & ((1u << g) - 1u));
    uint32_t v = p.fill;
    const bool kept = KEEP && p.src_of && p.src_of[(size_t)w * 64u + l] == wbs::kKeep;
    if (p.src && !kept) {
      uint32_t s = p.src_of ? p.src_of[(size_t)w * 64u + l] : w * 64u + l;
      if ((s >> 6) >= p.nwaves) s = w * 64u + l;   // (the host's plan: always in range)
      v = p.src[(size_t)(s >> 6) * p.words_s * 64u + wbh::lane_word(p.base_s + k, s & 63u, g)];
    }
    if (p.ls_fix) {
      const size_t slot = p.base_d + k;
      if (slot == LS_RPC) v = 0xFFFFFFFFu;
      else if (slot == LS_GSP || slot == LS_HBASE) v = 0u;
      else if (kept) continue;
    } else if (kept) {
      continue;
    }
    p.dst[(size_t)w * p.words_d * 64u + wbh::lane_word(p.base_d + k, l, g)] = v;
  }
}

// ---- the plan of a selective restore from a device map (SnapPlanParams) ---------------------
// A block of 64 threads per destination wave, thread t its lane t: what wbs::plan_restore does
// for the wave on the host. s_src, s_tiles, s_bad: 64 words of LDS each; the reductions over
// the wave go through them (no cross-lane operations: the text also runs as host code), and
// thread 0 folds the wave into the summary with the including file's
//   WB_SNAP_ATOMIC_MAX / _OR / _ADD(uint32_t *, uint32_t)
// An entry that is neither kKeep nor below n marks the map invalid (the caller then launches
// nothing else) and plans as a kept lane, so that nothing here indexes by it.
WB_SNAP_FN void snap_plan_body(const SnapPlanParams &p, uint32_t wave, uint32_t t, uint32_t *s_src,
                               uint32_t *s_tiles, uint32_t *s_bad) {
  if (wave >= p.nwaves || t >= 64u) return;
  const uint32_t i = wave * 64u + t;
  uint32_t s;
  bool bad = false;
  if (i < p.n) {
    s = p.map[i];
    bad = s != wbs::kKeep && s >= p.n;
  } else {   // (lane 0 of a wave is below n)
    const uint32_t s0 = p.map[wave * 64u];
    s = s0 == wbs::kKeep || s0 >= p.n ? wbs::kKeep : (s0 & ~63u) | t;
  }
  if (bad) s = wbs::kKeep;
  s_src[t] = s;
  s_tiles[t] = s != wbs::kKeep && (s >> 6) < p.nwaves ? p.snap_rows[s >> 6] / wbs::kTile : 0u;
  s_bad[t] = bad ? 1u : 0u;
  p.plan_src[i] = s;
  WB_SNAP_SYNC();
  if (t != 0) return;
  bool self = p.same_granule != 0, one = true;
  uint32_t tiles = 0, kept = 0, kept_n = 0, restored = 0, first = wbs::kKeep, low = 0;
  for (uint32_t l = 64; l-- > 0;)
    if (s_bad[l]) low = ~(wave * 64u + l);   // (descending: the lowest stays)
  for (uint32_t l = 0; l < 64; l++) {
    const uint32_t v = s_src[l];
    if (v == wbs::kKeep) {
      kept++;
      kept_n += wave * 64u + l < p.n ? 1u : 0u;
      continue;
    }
    restored += wave * 64u + l < p.n ? 1u : 0u;
    if (first == wbs::kKeep) first = v;
    self = self && v == wave * 64u + l;
    one = one && (v >> 6) == (first >> 6);
    tiles = s_tiles[l] > tiles ? s_tiles[l] : tiles;
  }
  const uint32_t cls = kept == 64u ? (uint32_t)wbs::kKeepAll
                                   : (self ? wbs::kIdentity : one ? wbs::kOneWave : wbs::kGather) |
                                         (kept ? wbs::kHasKeep : 0u);
  p.wave_plan[2u * wave] = cls;
  p.wave_plan[2u * wave + 1u] = tiles;
  if (low) WB_SNAP_ATOMIC_MAX(p.summary, low);
  if (kept_n) WB_SNAP_ATOMIC_OR(p.summary + 1, 1u);
  if (cls != wbs::kIdentity && cls != wbs::kKeepAll) WB_SNAP_ATOMIC_OR(p.summary + 2, 1u);
  if (restored) WB_SNAP_ATOMIC_ADD(p.summary + 3, restored);
}

// ---- the call stack of a suspended invocation (SnapStackParams) -----------------------------
// Rows of wave w the packed buffer holds, within the stack's depth now and within the buffer
// (the host's tables: always so).
WB_SNAP_FN uint32_t snap_stack_held(const SnapStackParams &p, uint32_t w) {
  const uint32_t r = p.snap_rows[w] < p.gs_depth ? p.snap_rows[w] : p.gs_depth;
  return p.snap_off[w] + (uint64_t)r * 64u <= p.snap_words ? r : 0u;
}

// capture (restore false) and the restore of a wave from itself: rows [0, held) of the wave
// between the stack and the packed buffer as they lie, 16 bytes per thread
WB_SNAP_FN void snap_stack_copy_body(const SnapStackParams &p, uint32_t b, uint32_t t, bool restore) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  const size_t pieces = (size_t)snap_stack_held(p, wave) * 16u;
  wb_snap_v4 *live = (wb_snap_v4 *)(p.gstack + (size_t)wave * p.gs_depth * 64u);
  wb_snap_v4 *held = (wb_snap_v4 *)(p.snap + p.snap_off[wave]);
  for (size_t i = (size_t)c * 256u + t; i < pieces; i += (size_t)p.chunks * 256u) {
    if (restore) live[i] = held[i];
    else held[i] = live[i];
  }
}

// restore through the source map: a wave of class kIdentity as above; of any other class,
// rows [0, the most its sources hold): a thread gathers one row's words of 4 adjacent lanes
// from their source lanes and stores them as one piece. A lane whose source wave holds fewer
// rows gets zero there (rows above a lane's depth are never read).
WB_SNAP_FN void snap_stack_fork_body(const SnapStackParams &p, uint32_t b, uint32_t t) {
  const uint32_t wave = b / p.chunks, c = b % p.chunks;
  if (wave >= p.nwaves) return;
  if (p.wave_plan[2u * wave] == wbs::kIdentity) {
    snap_stack_copy_body(p, b, t, true);
    return;
  }
  const uint32_t want = p.wave_plan[2u * wave + 1u];
  const size_t pieces = (size_t)(want < p.gs_depth ? want : p.gs_depth) * 16u;
  wb_snap_v4 *live = (wb_snap_v4 *)(p.gstack + (size_t)wave * p.gs_depth * 64u);
  for (size_t i = (size_t)c * 256u + t; i < pieces; i += (size_t)p.chunks * 256u) {
    const uint32_t r = (uint32_t)(i >> 4), l0 = 4u * ((uint32_t)i & 15u);
    wb_snap_v4 v;
    for (uint32_t q = 0; q < 4; q++) {
      uint32_t s = p.src[(size_t)wave * 64u + l0 + q];
      if ((s >> 6) >= p.nwaves) s = wave * 64u + l0 + q;   // (the host's plan: always in range)
      const uint32_t sw = s >> 6;
      v[q] = r < snap_stack_held(p, sw) ? p.snap[p.snap_off[sw] + (size_t)r * 64u + (s & 63u)] : 0u;
    }
    live[i] = v;
  }
}

// ---- the arrays indexed by instance (SnapInstParams) -----------------------------------------
// thread i of `stride` threads: status byte, count, hcall word and result row of instance x
// from its source's
WB_SNAP_FN void snap_inst_body(const SnapInstParams &p, size_t i, size_t stride) {
  for (size_t x = i; x < p.n; x += stride) {
    size_t s = p.src_of ? p.src_of[x] : x;
    if (s >= p.n) s = x;   // (the host's plan: always in range)
    p.status_d[x] = p.status_s[s];
    p.counts_d[x] = p.counts_s[s];
    p.hcall_d[x] = p.hcall_s[s];
    for (uint32_t k = 0; k < p.result_cells; k++)
      p.results_d[x * p.result_cells + k] = p.results_s[s * p.result_cells + k];
  }
}
