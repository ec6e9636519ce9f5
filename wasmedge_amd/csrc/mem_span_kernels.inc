// mem_span_kernels.inc -- the bodies of the device-resident spans transfer (mem_spans.hip wraps
// each in a __global__ function; DESIGN.md "Device-resident spans"). Plain vector loads and
// stores only. The including file defines
//   WB_SPAN_FN                    the function qualifiers (__device__ inline; host: inline)
//   WB_SPAN_SYNC()                the block barrier (__syncthreads(); host: a barrier)
//   WB_SPAN_BALLOT(pred, t)       the 64-bit mask of `pred` over the plan block's 64 threads
//   WB_SPAN_BCAST(v, lane, t)     thread `lane`'s v, in all 64 of them
//   WB_SPAN_ATOMIC_MIN / _ADD(uint32_t *, uint32_t)
// so that the same text runs as host code, a thread per GPU thread, under a sanitizer.
//
// The plan (a block of 64 threads per wave, thread t its lane t) reads every lane's two slots
// and its size, decides in range / out of bounds as mem_io.hip lane_span does, and classes the
// wave over the lanes that will move bytes. The move (a block of 256 threads per (wave, piece))
// reads the wave's class -- uniform over the block -- and runs the tile body or the per-lane
// body of mem_io.hip, the tile body from the wave's own start word. Every loop bound comes
// from Len: no slot value bounds a loop.

typedef uint32_t wb_span_v4 __attribute__((vector_size(16)));

constexpr uint32_t kSpanTile = wbp::kTileWords;
constexpr uint32_t kSpanPitch = kSpanTile + 1u;   // LDS row pitch, as mem_io.hip's tile
constexpr uint8_t kSpanOutOfBounds = 0x88;        // ErrCode::MemoryOutOfBounds

// The wave's region that holds word `w` of its lanes -- the reserved layout, or the pool row
// of w's page -- and w's index within it (*wl, for lane_word); nullptr: no such row
// (mem_io.hip region).
WB_SPAN_FN uint32_t *span_region(const MemSpanParams &p, uint32_t wave, uint32_t w, uint32_t *wl) {
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

WB_SPAN_FN uint8_t *span_row(const MemSpanParams &p, uint32_t inst) { return p.buf + (uint64_t)inst * p.stride; }

// bytes [0, nb) of `bytes` <-> bytes [sh/8, sh/8 + nb) of the memory word at `word`
template <bool WRITE>
WB_SPAN_FN void span_merge_bytes(uint32_t *word, uint8_t *bytes, uint32_t sh, uint32_t nb) {
  uint32_t v = *word;
  for (uint32_t q = 0; q < 4; q++) {
    if (q >= nb) break;
    const uint32_t s = sh + 8u * q;
    if (WRITE) v = (v & ~(0xFFu << s)) | ((uint32_t)bytes[q] << s);
    else bytes[q] = (uint8_t)(v >> s);
  }
  if (WRITE) *word = v;
}

// ---- the plan --------------------------------------------------------------------------------
WB_SPAN_FN void span_plan_body(const MemSpanParams &p, uint32_t wave, uint32_t t) {
  const uint32_t inst = wave * 64u + t;
  const bool valid = inst < p.n;
  uint32_t off = 0, len = p.len;
  if (valid && p.off_slots) off = (uint32_t)p.off_slots[(uint64_t)inst * p.off_stride];
  if (valid && p.len_slots) len = (uint32_t)p.len_slots[(uint64_t)inst * p.len_stride];
  const bool bad = valid && len > p.len;   // (the host then refuses the call: nothing moves)
  if (len > p.len) len = p.len;
  const uint64_t s = (uint64_t)p.offset + off, e = s + len;
  const uint32_t pages = p.lstate[((size_t)wave * p.ls_slots + LS_PAGES) * 64u + t];
  const bool ok = e <= ((uint64_t)pages << 16);   // memory.h:74-78
  const bool oob = valid && !ok, mover = valid && ok && len != 0;
  const uint32_t start = mover ? (uint32_t)s : 0u;   // (a mover: s < 2^32)
  p.lane_plan[2u * (size_t)inst] = oob ? wbp::kOob : start;
  p.lane_plan[2u * (size_t)inst + 1u] = mover ? len : 0u;
  // the class, over the movers
  const uint64_t mv = WB_SPAN_BALLOT(mover, t), ob = WB_SPAN_BALLOT(oob, t), bd = WB_SPAN_BALLOT(bad, t);
  const uint32_t first = mv ? (uint32_t)__builtin_ctzll(mv) : 0u;
  const uint32_t s0 = WB_SPAN_BCAST(start, first, t);
  const uint64_t differ = WB_SPAN_BALLOT(mover && start != s0, t);
  if (t != 0) return;
  if (wave == 0) {   // (nobody adds to the next call's summary before this kernel has ended)
    p.next_summary[0] = wbp::kNoBad;
    p.next_summary[1] = p.next_summary[2] = p.next_summary[3] = 0u;
  }
  uint32_t cls = wbp::kLane;
  if (!mv) cls = wbp::kNone;
  else if (!differ && (s0 & 15u) == 0 && p.align >= 16u) cls = wbp::kTile16;
  else if (!differ && (s0 & 3u) == 0 && p.align >= 4u) cls = wbp::kTile;
  p.wave_plan[2u * wave] = cls;
  p.wave_plan[2u * wave + 1u] = s0 >> 2;
  if (bd) WB_SPAN_ATOMIC_MIN(p.summary, wave * 64u + (uint32_t)__builtin_ctzll(bd));
  if (ob) WB_SPAN_ATOMIC_ADD(p.summary + 1, (uint32_t)__builtin_popcountll(ob));
  if (cls >= wbp::kTile) WB_SPAN_ATOMIC_ADD(p.summary + 2, 1u);
}

// ---- the move --------------------------------------------------------------------------------
// The status bytes and the write marks of a wave, by the block of its first piece: thread t <
// 64 its lane t; s_start / s_len hold the lane records.
WB_SPAN_FN void span_report(const MemSpanParams &p, uint32_t wave, uint32_t t, const uint32_t *s_start,
                            const uint32_t *s_len) {
  const uint32_t inst = wave * 64u + t;
  if (inst >= p.n) return;
  if (p.status) p.status[inst] = s_start[t] == wbp::kOob && !s_len[t] ? kSpanOutOfBounds : 0;
  if (p.write && s_len[t]) {
    const uint64_t e = (uint64_t)s_start[t] + s_len[t];
    uint32_t *mark = &p.lstate[((size_t)wave * p.ls_slots + LS_HWM) * 64u + t];
    if (e > *mark) *mark = e > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e;
  }
}

// The per-lane body (mem_io.hip wb_mem_io_lane_kernel). Piece c: word k = c * 64 + j of every
// lane's range, counted from the lane's own first word; thread t serves lane t & 63, words
// j = (t >> 6) + 4 * (0..15).
template <bool WRITE>
WB_SPAN_FN void span_lane_body(const MemSpanParams &p, uint32_t wave, uint32_t c, uint32_t t,
                               const uint32_t *s_start, const uint32_t *s_len) {
  const uint32_t lane = t & 63u, len = s_len[lane];
  if (!len) return;
  const uint64_t start = s_start[lane], end = start + len;
  const uint32_t fw = (uint32_t)(start >> 2), nwords = (uint32_t)((end + 3u) >> 2) - fw;
  uint8_t *row = span_row(p, wave * 64u + lane);
  for (uint32_t j = 0; j < kSpanTile / 4u; j++) {
    const uint32_t k = c * kSpanTile + (t >> 6) + 4u * j;
    if (k >= nwords) break;
    const uint32_t w = fw + k;
    uint32_t wl;
    uint32_t *reg = span_region(p, wave, w, &wl);
    if (!reg) continue;
    uint32_t *word = reg + wbh::lane_word(wl, lane, p.mlog);
    const uint64_t wb = (uint64_t)w << 2;
    const uint64_t lo = start > wb ? start : wb, hi = end < wb + 4u ? end : wb + 4u;
    uint8_t *bytes = row + (lo - start);
    if (hi - lo == 4u && ((uintptr_t)bytes & 3u) == 0) {
      if (WRITE) *word = *(const uint32_t *)bytes;
      else *(uint32_t *)bytes = *word;
    } else {
      span_merge_bytes<WRITE>(word, bytes, 8u * (uint32_t)(lo & 3u), (uint32_t)(hi - lo));
    }
  }
}

// The tile body (mem_io.hip wb_mem_io_tile_kernel). Piece ti: words [W0, W0 + 64) of the
// wave's 64 lanes, W0 = (sw & ~63) + 64 * ti, sw the wave's start word; word w of a lane is
// word w - sw of its row. tile: 64 * kSpanPitch words of LDS.
template <bool WRITE, bool ROW16>
WB_SPAN_FN void span_tile_body(const MemSpanParams &p, uint32_t wave, uint32_t ti, uint32_t sw, uint32_t t,
                               uint32_t *tile, const uint32_t *s_len) {
  const uint32_t g = p.mlog, gm = (1u << g) - 1u;
  const uint64_t at0 = (uint64_t)(sw & ~(kSpanTile - 1u)) + (uint64_t)ti * kSpanTile;
  if (at0 >= (1ull << 30)) return;   // (past every memory; uniform over the block)
  const uint32_t W0 = (uint32_t)at0;   // (so W0 + 64 and sw + len / 4 stay within 32 bits)
  uint32_t wl0;
  uint32_t *reg = span_region(p, wave, W0, &wl0);   // (uniform over the block)
  if (!reg) return;
  // word W0 + wi of `lane` goes through the tile: a whole word of its range
#define WB_IN_TILE(lane, wi) (W0 + (wi) >= sw && W0 + (wi) - sw < (s_len[lane] >> 2))
  // memory side: piece x / 4 of the tile's 16 KiB, elements x .. x + 3; element x is word
  // (x >> (6 + g) << g) + (x & gm) of lane (x >> g) & 63, at lane_word() of the two
#define WB_MEM_SIDE(BODY)                                                                    \
  for (uint32_t k = 0; k < 4; k++) {                                                         \
    const uint32_t x = 4u * (t + 256u * k);                                                  \
    uint32_t ln[4], wi[4];                                                                   \
    bool in[4];                                                                              \
    for (uint32_t q = 0; q < 4; q++) {                                                       \
      ln[q] = ((x + q) >> g) & 63u;                                                          \
      wi[q] = (((x + q) >> (6u + g)) << g) + ((x + q) & gm);                                 \
      in[q] = WB_IN_TILE(ln[q], wi[q]);                                                      \
    }                                                                                        \
    uint32_t *at = reg + wbh::lane_word(wl0 + wi[0], ln[0], g);   /* = tile region + x */    \
    BODY                                                                                     \
  }
  // buffer side: ROW16: words 4 * (t & 15) .. + 3 of rows (t >> 4) + 16 * (0..3);
  // else word t & 63 of rows (t >> 6) + 4 * (0..15)
#define WB_ROW_SIDE(BODY16, BODY4)                                                           \
  if (ROW16) {                                                                               \
    for (uint32_t k = 0; k < 4; k++) {                                                       \
      const uint32_t lane = (t >> 4) + 16u * k, wi = 4u * (t & 15u);                         \
      bool in[4];                                                                            \
      for (uint32_t q = 0; q < 4; q++) in[q] = WB_IN_TILE(lane, wi + q);                     \
      if (!(in[0] || in[1] || in[2] || in[3])) continue;                                     \
      uint32_t *at = (uint32_t *)span_row(p, wave * 64u + lane) + ((int64_t)W0 + wi - sw);   \
      uint32_t *cell = &tile[lane * kSpanPitch + wi];                                        \
      BODY16                                                                                 \
    }                                                                                        \
  } else {                                                                                   \
    for (uint32_t k = 0; k < 16; k++) {                                                      \
      const uint32_t lane = (t >> 6) + 4u * k, wi = t & 63u;                                 \
      if (!WB_IN_TILE(lane, wi)) continue;                                                   \
      uint32_t *at = (uint32_t *)span_row(p, wave * 64u + lane) + ((int64_t)W0 + wi - sw);   \
      uint32_t *cell = &tile[lane * kSpanPitch + wi];                                        \
      BODY4                                                                                  \
    }                                                                                        \
  }
  if (WRITE) {
    WB_ROW_SIDE(
        if (in[0] && in[1] && in[2] && in[3]) {
          const wb_span_v4 v = *(const wb_span_v4 *)at;
          cell[0] = v[0]; cell[1] = v[1]; cell[2] = v[2]; cell[3] = v[3];
        } else {
          for (uint32_t q = 0; q < 4; q++)
            if (in[q]) cell[q] = at[q];
        },
        *cell = *at;)
    WB_SPAN_SYNC();
    WB_MEM_SIDE(
        if (in[0] && in[1] && in[2] && in[3]) {
          wb_span_v4 v;
          v[0] = tile[ln[0] * kSpanPitch + wi[0]]; v[1] = tile[ln[1] * kSpanPitch + wi[1]];
          v[2] = tile[ln[2] * kSpanPitch + wi[2]]; v[3] = tile[ln[3] * kSpanPitch + wi[3]];
          *(wb_span_v4 *)at = v;
        } else {
          for (uint32_t q = 0; q < 4; q++)
            if (in[q]) at[q] = tile[ln[q] * kSpanPitch + wi[q]];
        })
  } else {
    WB_MEM_SIDE(
        if (in[0] || in[1] || in[2] || in[3]) {   // (the whole piece lies in the region)
          const wb_span_v4 v = *(const wb_span_v4 *)at;
          tile[ln[0] * kSpanPitch + wi[0]] = v[0]; tile[ln[1] * kSpanPitch + wi[1]] = v[1];
          tile[ln[2] * kSpanPitch + wi[2]] = v[2]; tile[ln[3] * kSpanPitch + wi[3]] = v[3];
        })
    WB_SPAN_SYNC();
    WB_ROW_SIDE(
        if (in[0] && in[1] && in[2] && in[3]) {
          wb_span_v4 v;
          v[0] = cell[0]; v[1] = cell[1]; v[2] = cell[2]; v[3] = cell[3];
          *(wb_span_v4 *)at = v;
        } else {
          for (uint32_t q = 0; q < 4; q++)
            if (in[q]) at[q] = cell[q];
        },
        *at = *cell;)
  }
  // a lane's last 1..3 bytes: its own word, past the words the tile moved
  if (t < 64 && (s_len[t] & 3u)) {
    const uint32_t w = sw + (s_len[t] >> 2);   // (sw < 2^30 and len / 4 < 2^30)
    if (w >= W0 && w < W0 + kSpanTile)
      span_merge_bytes<WRITE>(reg + wbh::lane_word(wl0 + (w - W0), t, g),
                              span_row(p, wave * 64u + t) + (s_len[t] & ~3u), 0, s_len[t] & 3u);
  }
#undef WB_ROW_SIDE
#undef WB_MEM_SIDE
#undef WB_IN_TILE
}

// Block b = (wave, piece) of p.nwaves * p.pieces; tile: 64 * kSpanPitch words of LDS, s_start
// and s_len: 64 words each. The caller put a barrier after the previous block's body.
template <bool WRITE>
WB_SPAN_FN void span_move_body(const MemSpanParams &p, uint64_t b, uint32_t t, uint32_t *tile,
                               uint32_t *s_start, uint32_t *s_len) {
  const uint32_t wave = (uint32_t)(b / p.pieces), c = (uint32_t)(b % p.pieces);
  if (wave >= p.nwaves) return;
  const uint32_t cls = p.wave_plan[2u * wave], sw = p.wave_plan[2u * wave + 1u];
  if (cls == wbp::kNone && c != 0) return;   // (the first piece still reports)
  if (t < 64) {
    s_start[t] = p.lane_plan[2u * ((size_t)wave * 64u + t)];
    s_len[t] = p.lane_plan[2u * ((size_t)wave * 64u + t) + 1u];
  }
  WB_SPAN_SYNC();
  if (c == 0 && t < 64) span_report(p, wave, t, s_start, s_len);
  if (cls == wbp::kTile16) span_tile_body<WRITE, true>(p, wave, c, sw, t, tile, s_len);
  else if (cls == wbp::kTile) span_tile_body<WRITE, false>(p, wave, c, sw, t, tile, s_len);
  else if (cls == wbp::kLane) span_lane_body<WRITE>(p, wave, c, t, s_start, s_len);
}
