// snapshot_rehearsal.cpp -- the snapshot kernel bodies (wasmedge_amd/csrc/snapshot_kernels.inc)
// as host code, a thread per GPU thread and a barrier for __syncthreads, against a per-lane
// word model (DESIGN.md "Selective restore"). Built with -fsanitize=address,undefined and run
// directly by tests/test_snapshot_select.py; prints "ok <cases>" and exits 0 when no word
// differs. No GPU, no library: only the headers the kernels themselves include.
//
//   snapshot_rehearsal            every case
//   snapshot_rehearsal <vector>   the cases of one keep vector
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
#include "snapshot.h"
#include "snapshot_plan.h"

static pthread_barrier_t *g_barrier = nullptr;

static inline void host_atomic_max(uint32_t *p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
}

#define WB_SNAP_FN inline
#define WB_SNAP_SYNC() pthread_barrier_wait(g_barrier)
#define WB_SNAP_ATOMIC_MAX(p, v) host_atomic_max((p), (v))
#define WB_SNAP_ATOMIC_OR(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#define WB_SNAP_ATOMIC_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)

namespace {

#include "snapshot_kernels.inc"

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

constexpr uint32_t N = 130, NW = 3, LANES = NW * 64, KEEP = 0xFFFFFFFFu;
constexpr uint32_t IMAGE_WORDS = 70, LS_SLOTS = 8;

uint32_t g_rng = 12345;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

std::vector<uint32_t> g_image;
uint32_t init_word(uint32_t w) { return w < IMAGE_WORDS ? g_image[w] : 0u; }

struct Named {
  std::string name;
  std::vector<uint32_t> map;
};

// the keep vectors of tests/test_snapshot_select.py (the fork's choice is the program's own:
// about 30% kept, the rest from [0, N / 2))
std::vector<Named> vectors() {
  std::vector<Named> v;
  auto make = [&](const char *name, const std::function<uint32_t(uint32_t)> &f) {
    Named x;
    x.name = name;
    for (uint32_t i = 0; i < N; i++) x.map.push_back(f(i));
    v.push_back(x);
  };
  make("none", [](uint32_t i) { return i; });
  make("all", [](uint32_t) { return KEEP; });
  make("waves", [](uint32_t i) { return i < 64 ? i : i < 128 ? KEEP : i == 128 ? KEEP : i; });
  make("waves2", [](uint32_t i) { return i < 64 ? i : i < 128 ? KEEP : i == 128 ? i : KEEP; });
  make("alternate", [](uint32_t i) { return i & 1 ? KEEP : i; });
  make("fork", [](uint32_t) { return rnd() % 10 < 3 ? KEEP : rnd() % (N / 2); });
  make("bcast", [](uint32_t i) { return i % 4 == 0 ? KEEP : 65u; });
  return v;
}

// the source of lane i of NW * 64 under the partial-wave rule, by the model's own words: a
// lane past N follows lane 0 of its wave into that lane's source wave, keeping its lane number,
// and is kept when that lane is
uint32_t model_source(const std::vector<uint32_t> &map, uint32_t i) {
  if (i < N) return map[i];
  const uint32_t lead = map[(i / 64) * 64];
  return lead == KEEP ? KEEP : (lead / 64) * 64 + i % 64;
}

uint32_t model_rows(uint32_t mark, uint32_t mem_words) {
  uint64_t need = (uint64_t(mark) + 3) / 4;
  if (need < IMAGE_WORDS) need = IMAGE_WORDS;
  uint64_t r = 0;
  while (r < need && r < mem_words) r += 64;
  return uint32_t(r < mem_words ? r : mem_words);
}

struct State {   // per-lane words and marks
  uint32_t mem_words = 0;
  std::vector<std::vector<uint32_t>> w;   // [LANES][mem_words]
  std::vector<uint32_t> mark;             // [LANES] bytes
};

State make_state(uint32_t mem_words, const std::function<uint32_t(uint32_t)> &mark_of) {
  State s;
  s.mem_words = mem_words;
  s.w.assign(LANES, std::vector<uint32_t>(mem_words));
  s.mark.resize(LANES);
  for (uint32_t l = 0; l < LANES; l++) {
    s.mark[l] = mark_of(l);
    for (uint32_t k = 0; k < mem_words; k++)
      s.w[l][k] = uint64_t(k) * 4 < s.mark[l] ? (rnd() | 1u) : init_word(k);
  }
  return s;
}

uint32_t wave_rows(const State &s, uint32_t wave, uint32_t mem_words) {
  uint32_t m = 0;
  for (uint32_t l = 0; l < 64; l++) m = s.mark[wave * 64 + l] > m ? s.mark[wave * 64 + l] : m;
  return model_rows(m, mem_words);
}

int g_failures = 0;
void fail(const std::string &what, const char *detail, uint64_t a, uint64_t b, uint64_t c) {
  if (g_failures++ < 20) printf("FAIL %s: %s %llu %llu %llu\n", what.c_str(), detail, (unsigned long long)a,
                                (unsigned long long)b, (unsigned long long)c);
}

// One memory-0 restore: a capture under (snap_words, gs), the live layout under (mem_words, gd).
void mem_case(const Named &v, uint32_t gs, uint32_t gd, uint32_t snap_words, uint32_t mem_words) {
  const std::string what = v.name + " gs=" + std::to_string(gs) + " gd=" + std::to_string(gd) + " words=" +
                           std::to_string(snap_words) + "/" + std::to_string(mem_words);
  // the capture: wave 0 low marks, wave 1 high ones (lane 70 the highest), wave 2 in between
  const State cap = make_state(snap_words, [](uint32_t l) {
    const uint32_t wv = l / 64;
    return wv == 0 ? rnd() % 1000 : wv == 1 ? (l == 70 ? 9000u : 3000 + rnd() % 3000) : 1500 + rnd() % 500;
  });
  // now: in wave 0 lanes 0..7 hold marks above every source's rows (kept ones among them under
  // every vector that keeps), one of them past the capture's layout where the layout doubled;
  // wave 2's marks are so low that its restored lanes' source rows lie above its current bound
  const bool doubled = mem_words > snap_words;
  const State now = make_state(mem_words, [&](uint32_t l) {
    const uint32_t wv = l / 64;
    if (wv == 0) return l < 8 ? (doubled && l == 3 ? snap_words * 4 + 1000 : 12000 + l * 64) : rnd() % 2000;
    return wv == 1 ? rnd() % 7000 : rnd() % 300;
  });
  // the packed snapshot and the live layout
  std::vector<uint32_t> rows(NW);
  std::vector<uint64_t> off(NW);
  uint64_t total = 0;
  for (uint32_t w = 0; w < NW; w++) {
    rows[w] = wave_rows(cap, w, snap_words);
    off[w] = total;
    total += uint64_t(rows[w]) * 64;
  }
  std::vector<uint32_t> snap(total + 4, 0xDEADBEEFu), mem(size_t(NW) * mem_words * 64);
  for (uint32_t l = 0; l < LANES; l++) {
    for (uint32_t k = 0; k < rows[l / 64]; k++) snap[off[l / 64] + wbh::lane_word(k, l % 64, gs)] = cap.w[l][k];
    for (uint32_t k = 0; k < mem_words; k++)
      mem[size_t(l / 64) * mem_words * 64 + wbh::lane_word(k, l % 64, gd)] = now.w[l][k];
  }
  std::vector<uint32_t> lstate(size_t(NW) * LS_SLOTS * 64, 0);
  for (uint32_t l = 0; l < LANES; l++) lstate[(size_t(l / 64) * LS_SLOTS + LS_HWM) * 64 + l % 64] = now.mark[l];
  // the plan (the library's) and the kernel the library would launch
  wbs::RestorePlan P;
  wbs::plan_restore(v.map.data(), N, NW, rows.data(), gs == gd, &P);
  SnapMemParams p{};
  p.mem = mem.data();
  p.snap = snap.data();
  p.snap_off = off.data();
  p.snap_rows = rows.data();
  p.lstate = lstate.data();
  p.image = g_image.data();
  p.src = P.src.data();
  p.wave_plan = P.wave.data();
  p.nwaves = NW;
  p.mem_words = mem_words;
  p.ls_slots = LS_SLOTS;
  p.image_words = IMAGE_WORDS;
  p.g_mem = gd;
  p.g_snap = gs;
  p.chunks = 3;
  std::vector<uint32_t> tile(64 * kSnapPitch), s_m(64), s_src(64), s_keep(64);
  // (a restore that keeps lanes launches the SELECT instantiations, any other the plain ones)
  if (P.identity && P.any_keep)
    launch(NW * p.chunks, 256, [&](uint32_t b, uint32_t t) { snap_restore_copy_body<true>(p, b, t, s_m.data()); });
  else if (P.identity)
    launch(NW * p.chunks, 256, [&](uint32_t b, uint32_t t) { snap_restore_copy_body<false>(p, b, t, s_m.data()); });
  else if (P.any_keep)
    launch(NW * p.chunks, 256, [&](uint32_t b, uint32_t t) {
      snap_select_gather_body(p, b, t, tile.data(), s_m.data(), s_src.data(), s_keep.data());
    });
  else
    launch(NW * p.chunks, 256, [&](uint32_t b, uint32_t t) {
      snap_restore_gather_body(p, b, t, tile.data(), s_m.data(), s_src.data());
    });
  // the model, lane by lane
  for (uint32_t l = 0; l < LANES; l++) {
    const uint32_t s = model_source(v.map, l), wv = l / 64;
    uint32_t newmark = now.mark[l];
    std::vector<uint32_t> want = now.w[l];
    if (s != KEEP) {
      // the wave's visit: the largest rows over its restored lanes' source waves, or its
      // current bound
      uint32_t visit = wave_rows(now, wv, mem_words);
      for (uint32_t m = 0; m < 64; m++) {
        const uint32_t sm = model_source(v.map, wv * 64 + m);
        if (sm != KEEP && rows[sm / 64] > visit) visit = rows[sm / 64];
      }
      for (uint32_t k = 0; k < visit && k < mem_words; k++) want[k] = k < rows[s / 64] ? cap.w[s][k] : init_word(k);
      newmark = cap.mark[s];
    }
    for (uint32_t k = 0; k < mem_words; k++) {
      const uint32_t got = mem[size_t(wv) * mem_words * 64 + wbh::lane_word(k, l % 64, gd)];
      if (got != want[k]) fail(what, "lane word got", l, k, got);
      // the write-mark argument: every word that differs from the image / zero lies below
      // the lane's new mark
      if (want[k] != init_word(k) && uint64_t(k) * 4 >= newmark) fail(what, "word above the new mark", l, k, newmark);
    }
  }
}

// The rows kernel over a [wave][words][64] buffer in granules of 2^g words.
void rows_case(const Named &v, uint32_t words_d, uint32_t words_s, uint32_t base_d, uint32_t base_s,
               uint32_t count, uint32_t g, bool fill, uint32_t ls_fix) {
  const std::string what = v.name + " rows " + std::to_string(words_d) + "/" + std::to_string(words_s) + " g=" +
                           std::to_string(g) + (fill ? " fill" : "") + (ls_fix ? " ls" : "");
  std::vector<uint32_t> dst(size_t(NW) * words_d * 64), src(size_t(NW) * words_s * 64), plan(LANES);
  for (auto &x : dst) x = rnd();
  for (auto &x : src) x = rnd();
  const std::vector<uint32_t> before = dst;
  bool any_keep = false;
  for (uint32_t l = 0; l < LANES; l++) {
    plan[l] = model_source(v.map, l);
    any_keep = any_keep || plan[l] == KEEP;
  }
  SnapRowsParams r{};
  r.dst = dst.data();
  r.src = fill ? nullptr : src.data();
  r.src_of = plan.data();
  r.nwaves = NW;
  r.words_d = words_d;
  r.words_s = fill ? 0 : words_s;
  r.base_d = base_d;
  r.base_s = base_s;
  r.count = count;
  r.g = g;
  r.fill = fill ? 0xFFFFFFFFu : 0u;
  r.ls_fix = ls_fix;
  r.keep = any_keep ? 1 : 0;
  for (size_t i = 0; i < 256; i++) {
    if (any_keep) snap_rows_body<true>(r, i, 256);
    else snap_rows_body<false>(r, i, 256);
  }
  for (uint32_t l = 0; l < LANES; l++)
    for (uint32_t k = 0; k < words_d; k++) {
      const size_t at = size_t(l / 64) * words_d * 64 + wbh::lane_word(k, l % 64, g);
      uint32_t want = before[at];
      const bool inside = k >= base_d && k < base_d + count;
      if (inside && plan[l] != KEEP)
        want = fill ? 0xFFFFFFFFu
                    : src[size_t(plan[l] / 64) * words_s * 64 + wbh::lane_word(base_s + (k - base_d), plan[l] % 64, g)];
      if (inside && ls_fix) {
        if (k == LS_RPC) want = 0xFFFFFFFFu;
        if (k == LS_GSP || k == LS_HBASE) want = 0u;
      }
      if (dst[at] != want) fail(what, "lane word got", l, k, dst[at]);
    }
}

// The plan kernel's body against wbs::plan_restore.
void plan_case(const Named &v, bool same, const std::vector<uint32_t> &rows) {
  const std::string what = v.name + " plan same=" + std::to_string(same);
  wbs::RestorePlan P;
  wbs::plan_restore(v.map.data(), N, NW, rows.data(), same, &P);
  std::vector<uint32_t> src(LANES, 0x55555555u), wave(NW * 2, 0x55555555u), sum(4, 0);
  std::vector<uint32_t> a(64), b(64), c(64);
  SnapPlanParams q{};
  q.map = v.map.data();
  q.snap_rows = rows.data();
  q.plan_src = src.data();
  q.wave_plan = wave.data();
  q.summary = sum.data();
  q.n = N;
  q.nwaves = NW;
  q.same_granule = same ? 1 : 0;
  launch(NW, 64, [&](uint32_t blk, uint32_t t) { snap_plan_body(q, blk, t, a.data(), b.data(), c.data()); });
  if (src != P.src) fail(what, "plan_src differs", 0, 0, 0);
  if (wave != P.wave) fail(what, "wave_plan differs", wave[0], wave[2], wave[4]);
  if (sum[0] != 0 || (sum[1] != 0) != P.any_keep || (sum[2] != 0) != !P.identity || sum[3] != P.restored)
    fail(what, "summary", sum[1], sum[2], sum[3]);
}

}  // namespace

int main(int argc, char **argv) {
  for (uint32_t k = 0; k < IMAGE_WORDS; k++) g_image.push_back(k % 9 == 0 ? 0u : rnd());
  const std::vector<Named> vs = vectors();
  const uint32_t granules[4] = {0, 1, 2, 5};   // 4, 8, 16 and 128 bytes
  const uint32_t W = 4096;   // words per lane of the capture's layout: room for every mark below
  int cases = 0;
  for (const Named &v : vs) {
    if (argc > 1 && v.name != argv[1]) continue;
    for (uint32_t g : granules) {
      mem_case(v, g, g, W, W);                   // the layout of the capture
      mem_case(v, g, g, W, 2 * W);               // the reserved layout doubled since
      mem_case(v, g == 0 ? 5 : 0, g, W, W);      // the granule changed since
      cases += 3;
    }
    // instance state (LS_RPC / LS_GSP / LS_HBASE rewritten, kept lanes included); a table
    // widened since the capture, its copy and its fill; memories 1..7 in 16-byte granules
    rows_case(v, LS_SLOTS, LS_SLOTS, 0, 0, LS_SLOTS, 0, false, 1);
    rows_case(v, LS_SLOTS, LS_SLOTS, 0, 0, LS_SLOTS, 0, false, 0);
    rows_case(v, 12, 6, 2, 1, 4, 0, false, 0);
    rows_case(v, 12, 6, 6, 0, 5, 0, true, 0);
    rows_case(v, 16, 16, 0, 0, 16, 2, false, 0);
    for (int same = 0; same < 2; same++) plan_case(v, same != 0, {128, 2304, 512});
    cases += 7;
  }
  if (argc <= 1) {   // an invalid map: the summary names the lowest bad entry
    std::vector<uint32_t> map(N), src(LANES), wave(NW * 2), sum(4, 0), rows = {128, 2304, 512};
    std::vector<uint32_t> a(64), b(64), c(64);
    for (uint32_t i = 0; i < N; i++) map[i] = i;
    map[70] = N;
    map[5] = 0xFFFFFFFEu;
    map[129] = 0x80000000u;
    SnapPlanParams q{};
    q.map = map.data();
    q.snap_rows = rows.data();
    q.plan_src = src.data();
    q.wave_plan = wave.data();
    q.summary = sum.data();
    q.n = N;
    q.nwaves = NW;
    q.same_granule = 1;
    launch(NW, 64, [&](uint32_t blk, uint32_t t) { snap_plan_body(q, blk, t, a.data(), b.data(), c.data()); });
    if (sum[0] != ~5u) fail("invalid map", "summary names", ~sum[0], 0, 0);
    cases++;
  }
  if (g_failures) {
    printf("%d differing words or plans\n", g_failures);
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}
