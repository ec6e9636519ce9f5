// memspans_rehearsal.cpp -- the plan and move bodies of the device-resident spans transfer
// (wasmedge_amd/csrc/mem_span_kernels.inc) as host code, a thread per GPU thread and a barrier
// for __syncthreads, against a per-lane byte model (DESIGN.md "Device-resident spans"). Built
// with -fsanitize=address,undefined and run directly by tests/test_memspans.py; prints
// "ok <cases>" and exits 0 when no byte, status, write mark or summary word differs. No GPU, no
// library: only the headers the kernels themselves include.
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "kparams.h"
#include "mem_layout.h"
#include "mem_spans.h"

static pthread_barrier_t *g_barrier = nullptr;
static uint32_t g_flag[64], g_val[64];   // the plan block's cross-lane scratch

static inline void host_atomic_min(uint32_t *p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
}
static inline uint64_t host_ballot(bool pred, uint32_t t) {
  g_flag[t] = pred ? 1u : 0u;
  pthread_barrier_wait(g_barrier);
  uint64_t m = 0;
  for (uint32_t l = 0; l < 64; l++) m |= uint64_t(g_flag[l]) << l;
  pthread_barrier_wait(g_barrier);
  return m;
}
static inline uint32_t host_bcast(uint32_t v, uint32_t lane, uint32_t t) {
  g_val[t] = v;
  pthread_barrier_wait(g_barrier);
  const uint32_t r = g_val[lane];
  pthread_barrier_wait(g_barrier);
  return r;
}

#define WB_SPAN_FN inline
#define WB_SPAN_SYNC() pthread_barrier_wait(g_barrier)
#define WB_SPAN_BALLOT(pred, t) host_ballot((pred), (t))
#define WB_SPAN_BCAST(v, lane, t) host_bcast((v), (lane), (t))
#define WB_SPAN_ATOMIC_MIN(p, v) host_atomic_min((p), (v))
#define WB_SPAN_ATOMIC_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)

namespace {

#include "mem_span_kernels.inc"

// `grid` blocks of `threads` threads, one block after the other (the LDS arrays are the
// caller's, shared by the blocks in turn): fn(block, thread)
void launch(uint32_t grid, uint32_t threads, const std::function<void(uint32_t, uint32_t)> &fn) {
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, threads);
  g_barrier = &bar;
  struct Arg {
    const std::function<void(uint32_t, uint32_t)> *fn;
    uint32_t grid, t;
    pthread_barrier_t *bar;
  };
  std::vector<Arg> args(threads);
  std::vector<pthread_t> th(threads);
  for (uint32_t t = 0; t < threads; t++) {
    args[t] = Arg{&fn, grid, t, &bar};
    pthread_create(&th[t], nullptr, [](void *v) -> void * {
      const Arg *a = static_cast<const Arg *>(v);
      for (uint32_t b = 0; b < a->grid; b++) {
        (*a->fn)(b, a->t);
        pthread_barrier_wait(a->bar);   // (the next block reuses the LDS arrays)
      }
      return nullptr;
    }, &args[t]);
  }
  for (uint32_t t = 0; t < threads; t++) pthread_join(th[t], nullptr);
  pthread_barrier_destroy(&bar);
  g_barrier = nullptr;
}

constexpr uint32_t N = 130, NW = 3, LANES = NW * 64, LS_SLOTS = LS_GLOBALS;
constexpr uint32_t PAGE = 65536, PAGE_WORDS = 16384;

uint32_t g_rng = 2463534242u;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

int g_failures = 0;
void fail(const std::string &what, const char *detail, uint64_t a, uint64_t b, uint64_t c) {
  if (g_failures++ < 20) printf("FAIL %s: %s %llu %llu %llu\n", what.c_str(), detail, (unsigned long long)a,
                                (unsigned long long)b, (unsigned long long)c);
}

struct Case {
  std::string name;
  uint32_t rpages, pool_pages;                 // the reserved layout; pool pages a wave can name
  std::function<uint32_t(uint32_t)> pages;     // of instance i (<= rpages + pool_pages)
  uint32_t offset, len;
  uint64_t stride;
  uint32_t shift;                              // the rows' buffer starts this many bytes past 16-byte alignment
  std::function<int64_t(uint32_t)> own;        // instance i's own offset; nullptr: no OffsetSlots
  std::function<int64_t(uint32_t)> own_len;    // its length; nullptr: no LenSlots
  uint64_t slot_stride;
  bool status;
  int tiled;                                   // the tiled waves the case is built for (-1: the model's)
  bool every_granule;                          // false: the 4-byte and the 128-byte granule only
};

// the word of lane l at word address k before the transfer
uint32_t fresh_word(uint32_t l, uint32_t k) { return (k * 2654435761u) ^ (l * 0x9E3779B9u) ^ 0x5bd1e995u; }

void run_case(const Case &c, uint32_t g) {
  const std::string what = c.name + " g=" + std::to_string(g);
  const uint32_t mem_words = c.rpages * PAGE_WORDS;
  // the model: bytes of every lane; the device form: the reserved layout and the pool rows
  std::vector<uint32_t> pages(LANES, 0);
  for (uint32_t l = 0; l < LANES; l++) pages[l] = c.pages(l < N ? l : N - 1);
  std::vector<std::vector<uint8_t>> model(LANES);
  std::vector<uint32_t> mem(size_t(NW) * mem_words * 64);
  std::vector<std::vector<uint32_t>> rows_of_pool;   // each 64 lanes x 16384 words
  std::vector<uint64_t> ptab(size_t(NW) * (c.pool_pages ? c.pool_pages : 1), 0);
  for (uint32_t w = 0; w < NW; w++) {
    uint32_t most = 0;
    for (uint32_t l = 0; l < 64; l++) most = pages[w * 64 + l] > most ? pages[w * 64 + l] : most;
    for (uint32_t k = 0; c.rpages + k < most; k++) {
      rows_of_pool.emplace_back(size_t(64) * PAGE_WORDS);
      ptab[size_t(w) * c.pool_pages + k] = uint64_t(uintptr_t(rows_of_pool.back().data()));
    }
  }
  auto word_at = [&](uint32_t l, uint32_t k) -> uint32_t * {
    const uint32_t w = l / 64, page = k / PAGE_WORDS;
    if (page < c.rpages) return &mem[size_t(w) * mem_words * 64 + wbh::lane_word(k, l % 64, g)];
    const uint64_t a = ptab[size_t(w) * c.pool_pages + (page - c.rpages)];
    return a ? reinterpret_cast<uint32_t *>(uintptr_t(a)) + wbh::lane_word(k % PAGE_WORDS, l % 64, g) : nullptr;
  };
  for (uint32_t l = 0; l < LANES; l++) {
    model[l].resize(size_t(pages[l]) * PAGE);
    for (uint32_t k = 0; k < pages[l] * PAGE_WORDS; k++) {
      const uint32_t v = fresh_word(l, k);
      memcpy(&model[l][size_t(k) * 4], &v, 4);
      *word_at(l, k) = v;
    }
  }
  std::vector<uint32_t> lstate(size_t(NW) * LS_SLOTS * 64, 0);
  auto ls = [&](uint32_t l, uint32_t slot) -> uint32_t & { return lstate[(size_t(l / 64) * LS_SLOTS + slot) * 64 + l % 64]; };
  for (uint32_t l = 0; l < LANES; l++) {
    ls(l, LS_PAGES) = pages[l];
    ls(l, LS_HWM) = 100 + l;
  }
  // the slots: garbage in the upper halves, and in the slots between the columns
  std::vector<uint64_t> off_slots, len_slots;
  auto slots = [&](std::vector<uint64_t> &v, const std::function<int64_t(uint32_t)> &f) {
    v.assign(size_t(N - 1) * c.slot_stride + 1, 0xDEADBEEFCAFEF00Dull);
    for (uint32_t i = 0; i < N; i++) v[size_t(i) * c.slot_stride] = (uint64_t(0xDEADBEEFu) << 32) | uint32_t(f(i));
  };
  if (c.own) slots(off_slots, c.own);
  if (c.own_len) slots(len_slots, c.own_len);
  // what the model expects of every instance
  std::vector<uint64_t> start(N);
  std::vector<uint32_t> len(N);
  std::vector<uint8_t> oob(N);
  uint32_t n_oob = 0, lowest_bad = wbp::kNoBad;
  for (uint32_t i = 0; i < N; i++) {
    start[i] = uint64_t(c.offset) + (c.own ? uint32_t(c.own(i)) : 0u);
    len[i] = c.own_len ? uint32_t(c.own_len(i)) : c.len;
    if (len[i] > c.len && lowest_bad == wbp::kNoBad) lowest_bad = i;
    if (len[i] > c.len) len[i] = c.len;
    oob[i] = start[i] + len[i] > uint64_t(pages[i]) * PAGE;
    n_oob += oob[i];
  }
  const uintptr_t bits = uintptr_t(c.shift) | uintptr_t(c.stride);
  const uint32_t align = bits % 16 == 0 ? 16 : bits % 4 == 0 ? 4 : 1;
  uint32_t tiled = 0;
  for (uint32_t w = 0; w < NW; w++) {
    bool any = false, same = true;
    uint64_t s0 = 0;
    for (uint32_t i = w * 64; i < N && i < w * 64 + 64; i++) {
      if (oob[i] || !len[i]) continue;
      if (!any) s0 = start[i];
      any = true;
      same = same && start[i] == s0;
    }
    tiled += any && same && s0 % 4 == 0 && align >= 4;
  }
  if (c.tiled >= 0 && uint32_t(c.tiled) != tiled) fail(what, "the model's tiled waves are not the case's", tiled, c.tiled, 0);

  const size_t row_bytes = size_t(N) * c.stride;
  std::vector<uint8_t> raw(row_bytes + 64), status(N), given(row_bytes + 1);
  uint8_t *buf = raw.data() + ((16 - uintptr_t(raw.data()) % 16) % 16) + c.shift;
  std::vector<uint32_t> lane_plan(size_t(LANES) * 2), wave_plan(NW * 2), sum(4), next_sum(4), tile(64 * kSpanPitch), s_a(64), s_b(64);
  MemSpanParams p{};
  p.mem = mem.data();
  p.lstate = lstate.data();
  p.ptab = c.pool_pages ? ptab.data() : nullptr;
  p.off_slots = c.own ? off_slots.data() : nullptr;
  p.len_slots = c.own_len ? len_slots.data() : nullptr;
  p.buf = c.len ? buf : nullptr;
  p.status = c.status ? status.data() : nullptr;
  p.lane_plan = lane_plan.data();
  p.wave_plan = wave_plan.data();
  p.summary = sum.data();
  p.next_summary = next_sum.data();
  p.off_stride = p.len_stride = c.slot_stride;
  p.stride = c.len ? c.stride : 0;
  p.mem_words = mem_words;
  p.mlog = g;
  p.ptab_w = c.pool_pages;
  p.ls_slots = LS_SLOTS;
  p.n = N;
  p.nwaves = NW;
  p.offset = c.offset;
  p.len = c.len;
  p.align = align;
  p.pieces = wbp::pieces_of(c.len);

  for (int write = 1; write >= 0; write--) {
    const std::string dir = what + (write ? " write" : " read");
    p.write = uint32_t(write);
    for (size_t k = 0; k < row_bytes; k++) given[k] = write ? uint8_t(rnd() | 1u) : 0x77;
    memcpy(buf, given.data(), row_bytes);
    memset(status.data(), 0x77, N);
    const std::vector<uint32_t> lstate0 = lstate;
    sum = {wbp::kNoBad, 0, 0, 0};
    next_sum = {1, 2, 3, 4};
    launch(NW, 64, [&](uint32_t b, uint32_t t) { span_plan_body(p, b, t); });
    if (sum[0] != lowest_bad || sum[1] != n_oob || sum[2] != tiled || sum[3] != 0)
      fail(dir, "summary", sum[0], sum[1], sum[2]);
    if (next_sum != std::vector<uint32_t>{wbp::kNoBad, 0, 0, 0}) fail(dir, "the next call's summary", next_sum[0], next_sum[1], next_sum[2]);
    // the plan writes nothing a caller can see; a refused call stops here
    if (memcmp(buf, given.data(), row_bytes) != 0 || lstate != lstate0) fail(dir, "the plan touched rows or state", 0, 0, 0);
    for (uint32_t i = 0; i < N; i++)
      if (status[i] != 0x77) fail(dir, "the plan touched a status byte", i, status[i], 0);
    if (lowest_bad == wbp::kNoBad) {
      launch(NW * p.pieces, 256, [&](uint32_t b, uint32_t t) {
        if (write) span_move_body<true>(p, b, t, tile.data(), s_a.data(), s_b.data());
        else span_move_body<false>(p, b, t, tile.data(), s_a.data(), s_b.data());
      });
      std::vector<uint8_t> want = given;
      for (uint32_t i = 0; i < N; i++) {
        if (c.status && status[i] != (oob[i] ? 0x88 : 0)) fail(dir, "status", i, status[i], oob[i]);
        uint32_t mark = 100 + i;
        if (!oob[i] && len[i]) {
          if (write) {
            memcpy(&model[i][start[i]], given.data() + size_t(i) * c.stride, len[i]);
            if (start[i] + len[i] > mark) mark = uint32_t(start[i] + len[i]);
          } else {
            memcpy(want.data() + size_t(i) * c.stride, &model[i][start[i]], len[i]);
          }
        }
        if (write) ls(i, LS_HWM) = ls(i, LS_HWM) == mark ? 100 + i : 0xBADu;   // (back to the start, or flagged)
      }
      if (lstate != lstate0) fail(dir, "write marks or instance state", 0, 0, 0);
      if (memcmp(buf, want.data(), row_bytes) != 0) {
        size_t k = 0;
        while (buf[k] == want[k]) k++;
        fail(dir, "row byte", k / c.stride, k % c.stride, buf[k]);
      }
    }
    if (!c.status)
      for (uint32_t i = 0; i < N; i++)
        if (status[i] != 0x77) fail(dir, "a status byte without PerInstance", i, status[i], 0);
    for (uint32_t l = 0; l < LANES; l++)
      for (uint32_t k = 0; k < pages[l] * PAGE_WORDS; k++) {
        uint32_t v;
        memcpy(&v, &model[l][size_t(k) * 4], 4);
        if (*word_at(l, k) != v) {
          fail(dir, "memory word of lane", l, k, *word_at(l, k));
          break;
        }
      }
  }
}

}  // namespace

int main() {
  auto all = [](uint32_t pg) { return [pg](uint32_t) { return pg; }; };
  auto uni = [](int64_t v) { return [v](uint32_t) { return v; }; };
  auto grown = [](uint32_t i) { return 1 + i % 3; };
  auto mixed = [](uint32_t i) -> int64_t { return i < 64 ? 512 : i < 128 ? int64_t((i * 37) % 509) : 8; };
  const std::vector<Case> cases = {
      // name, rpages, pool, pages, Offset, Len, Stride, shift, own, own_len, slot stride, status, tiled, every granule
      {"uniform aligned", 1, 0, all(1), 256, 4096, 4096, 0, uni(1024), nullptr, 1, true, 3, true},
      {"uniform aligned, 4-byte rows", 1, 0, all(1), 256, 1028, 1032, 4, uni(1024), nullptr, 3, true, 3, true},
      {"no slots", 1, 0, all(1), 260, 1000, 1000, 0, nullptr, nullptr, 1, true, 3, false},
      {"mixed", 1, 0, all(1), 0, 1000, 1000, 0, mixed, nullptr, 3, true, 2, true},
      {"uniform unaligned", 1, 0, all(1), 3, 1001, 1004, 0, uni(1024), nullptr, 1, true, 0, true},
      {"unaligned rows", 1, 0, all(1), 256, 1000, 1001, 0, uni(1024), nullptr, 1, true, 0, false},
      {"lengths", 1, 0, all(1), 0, 67, 68, 0, uni(2048), [](uint32_t i) -> int64_t { return i % 68; }, 2, true, 3, true},
      {"lengths, per lane", 1, 0, all(1), 3, 67, 70, 0, mixed, [](uint32_t i) -> int64_t { return i % 68; }, 2, true, 0, true},
      {"zero Len", 1, 0, all(1), 65536, 0, 0, 0, nullptr, nullptr, 1, true, 0, false},
      {"zero Len past the end", 1, 0, all(1), 65536, 0, 0, 0, uni(1), nullptr, 1, true, 0, false},
      {"out of bounds in a uniform wave", 1, 3, grown, 0, 4096, 4096, 0, uni(PAGE - 128), nullptr, 1, true, 3, true},
      {"out of bounds, no status", 1, 3, grown, 64, 256, 256, 0, uni(2 * PAGE - 128), nullptr, 1, false, 3, true},
      {"pool boundary", 1, 3, all(3), PAGE - 128, 4096, 4096, 0, uni(0), nullptr, 1, true, 3, true},
      {"second pool boundary", 1, 3, all(3), 0, 4096, 4100, 8, uni(2 * PAGE - 64), nullptr, 1, true, 3, true},
      {"pool boundary, per lane", 1, 3, all(3), PAGE - 300, 700, 700, 0, mixed, nullptr, 1, true, 2, false},
      {"start past 4 GiB", 1, 0, all(1), 0xFFFFFFF0u, 16, 16, 0, uni(0x100), nullptr, 1, true, 0, false},
      {"the last bytes", 1, 0, all(1), PAGE - 4099, 4099, 4100, 0, uni(0), nullptr, 1, true, 0, false},
      {"the last words", 1, 0, all(1), PAGE - 4100, 4099, 4100, 0, uni(0), nullptr, 1, true, 3, false},
      {"a length past Len", 1, 0, all(1), 0, 8, 8, 0, uni(64),
       [](uint32_t i) -> int64_t { return i == 77 || i == 5 ? 9 : 8; }, 1, true, 3, true},
  };
  const uint32_t granules[4] = {0, 1, 2, 5};   // 4, 8, 16 and 128 bytes
  int count = 0;
  for (const Case &c : cases)
    for (uint32_t g : granules) {
      if (!c.every_granule && g != 0 && g != 5) continue;
      run_case(c, g);
      count++;
    }
  if (g_failures) {
    printf("%d differences\n", g_failures);
    return 1;
  }
  printf("ok %d\n", count);
  return 0;
}
