// snapshot.cpp -- instance snapshots (WasmEdge_BatchSnapshotCreate / Restore / GetBytes /
// Delete; DESIGN.md "Instance snapshots"): the state of every instance as it stands between
// runs, held on the device, and a restore that starts instance i from the captured state of
// instance SrcOf[i]. WasmEdge_BatchSnapshotCreateSuspended (DESIGN.md "Snapshots of suspended
// runs") also holds the suspended invocation of a resumable context -- frames, call stack,
// resume points, statuses, counts and result rows --, which a restore reinstates for
// BatchResume. The device side is snapshot.hip; the planning that needs no device is
// snapshot_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "batch_ctx.h"
#include "multi.h"
#include "snapshot.h"
#include "snapshot_plan.h"

extern "C" hipError_t wb_launch_snap_mem(const SnapMemParams *p, int kind, hipStream_t s);
extern "C" hipError_t wb_launch_snap_rows(const SnapRowsParams *p, hipStream_t s);
extern "C" hipError_t wb_launch_snap_plan(const SnapPlanParams *p, hipStream_t s);
extern "C" hipError_t wb_launch_snap_stack(const SnapStackParams *p, int kind, hipStream_t s);
extern "C" hipError_t wb_launch_snap_inst(const SnapInstParams *p, hipStream_t s);

using namespace wbh;
using Ctx = WasmEdge_BatchContext;

struct WasmEdge_BatchSnapshot {
  Ctx *ctx = nullptr;   // the context it was taken from; NULL once that was deleted (inert)
  int device = 0;
  std::vector<WasmEdge_BatchSnapshot *> subs;   // a multi-device context's: one per shard
  // the layout it was taken under (a restore translates to the context's current one)
  uint32_t n = 0, nwaves = 0, mlog = 0, mem_words = 0, ls_slots = 0, tab_words = 0, xlog = 0, xwords = 0;
  std::vector<uint32_t> tabinfo;
  // memory 0: rows [0, rows_h[w]) of wave w at word off[w] of `mem` (snapshot_plan.h pack_rows)
  std::vector<uint32_t> rows_h;
  uint32_t max_tiles = 0;
  DevBuf<uint32_t> mem, rows;
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> lstate, ltab, xmem, xpages;   // copied whole
  std::vector<wbw::Lane> wasi;
  uint64_t bytes = 0;
  // the suspended invocation (CreateSuspended). Device: the frame-save rows, the HBM rows of
  // the call stack that parked lanes own -- rows [0, gs_rows_h[w]) of wave w at word gs_off[w]
  // of `gs` (snapshot_plan.h pack_stack) --, and the arrays indexed by instance. Host: the
  // invocation's descriptor and which instances were suspended.
  bool has_inv = false;
  uint32_t gs_depth = 0;          // the stack's depth at the capture
  uint64_t gs_words = 0;
  std::vector<uint32_t> gs_rows_h;
  DevBuf<uint32_t> gs, gs_rows, fsave, hcall, results;
  DevBuf<uint64_t> gs_off, counts;
  DevBuf<uint8_t> status;
  std::vector<uint8_t> susp_h;    // [n] 1: suspended (parked with WB_SUSPENDED in hcall)
  uint32_t suspended = 0;         // their number
  wbh::Staging staged;            // the staging it ran under (call_func / call_status current)
  uint32_t inv_pc = 0;
  // the last restore's plan and its device copy (kept here so that an untimed restore leaves
  // nothing of its own to free while its kernels run)
  mutable wbs::RestorePlan plan;
  mutable DevBuf<uint32_t> plan_src, plan_wave;
  mutable DevBuf<uint32_t> plan_sum;       // a device map's plan: the summary (SnapPlanParams)
  mutable std::vector<uint32_t> gs_plan;   // (snapshot_plan.h plan_stack)
  mutable DevBuf<uint32_t> gs_plan_d;
};
using Snap = WasmEdge_BatchSnapshot;

namespace wbs {

static std::mutex g_mu;   // the contexts' lists of their snapshots

void orphan(Ctx *C) {
  std::lock_guard<std::mutex> g(g_mu);
  for (Snap *s : C->snaps) s->ctx = nullptr;
  C->snaps.clear();
}

}  // namespace wbs

namespace {

// blocks per wave for the memory kernels: enough blocks to fill the device when the batch
// has few waves, no more than the tiles there are
uint32_t chunks_for(uint32_t nwaves, uint32_t max_tiles) {
  const uint32_t cap = std::max<uint32_t>(8, 4096 / std::max<uint32_t>(nwaves, 1));
  return std::min(std::max<uint32_t>(max_tiles, 1), cap);
}

// one LS slot of every lane, [nwaves][64], with one strided copy (as Reset fetches the pages)
bool fetch_slot(Ctx *C, uint32_t slot, std::vector<uint32_t> *out) {
  const size_t row = 64 * sizeof(uint32_t), pitch = size_t(C->ls_slots) * row;
  out->assign(size_t(C->nwaves) * 64, 0);
  return C->hip_ok(hipMemcpy2D(out->data(), row, C->lstate.ptr + size_t(slot) * 64, pitch, row, C->nwaves,
                               hipMemcpyDeviceToHost), "instance state");
}

template <typename T>
bool copy_whole(Ctx *C, DevBuf<T> *to, const DevBuf<T> &from, size_t count, uint64_t *bytes) {
  if (!count) return true;
  if (!to->alloc(count)) {
    (void)hipGetLastError();
    C->last_error = "snapshot: no device memory";
    return false;
  }
  *bytes += count * sizeof(T);
  return C->hip_ok(hipMemcpyAsync(to->ptr, from.ptr, count * sizeof(T), hipMemcpyDeviceToDevice, C->stream),
                   "snapshot");
}

// rows of the call stack per block column: as chunks_for, a tile's worth of rows per step
uint32_t stack_chunks(uint32_t nwaves, const std::vector<uint32_t> &rows) {
  uint32_t most = 0;
  for (uint32_t r : rows) most = std::max(most, (r + wbs::kTile - 1) / wbs::kTile);
  return chunks_for(nwaves, most);
}

// The suspended invocation of a resumable context into S (the caller checked inv_live and
// waited for the stream): every lane's LS_RPC / LS_GSP bound the call-stack rows to hold;
// the state slots themselves are in S->lstate already.
bool capture_invocation(Ctx *C, Snap *S) {
  std::vector<uint32_t> rpc, gsp, hc(C->n);
  std::vector<uint64_t> off;
  if (!fetch_slot(C, LS_RPC, &rpc) || !fetch_slot(C, LS_GSP, &gsp)) return false;
  S->gs_depth = C->gs_depth;
  S->gs_words = wbs::pack_stack(rpc.data(), gsp.data(), C->n, C->nwaves, C->gs_lds, C->gs_depth, &S->gs_rows_h, &off);
  if (!S->gs.alloc(size_t(S->gs_words) + 4) || !S->gs_rows.upload(S->gs_rows_h, C->stream) ||
      !S->gs_off.upload(off, C->stream)) {
    (void)hipGetLastError();
    C->last_error = "snapshot: no device memory";
    return false;
  }
  S->bytes += (S->gs_words + 4) * 4 + uint64_t(C->nwaves) * 12;
  SnapStackParams p{};
  p.gstack = C->gstack.ptr;
  p.snap = S->gs.ptr;
  p.snap_off = S->gs_off.ptr;
  p.snap_rows = S->gs_rows.ptr;
  p.snap_words = S->gs_words;
  p.nwaves = C->nwaves;
  p.gs_depth = C->gs_depth;
  p.chunks = stack_chunks(C->nwaves, S->gs_rows_h);
  if (!C->hip_ok(wb_launch_snap_stack(&p, 0, C->stream), "snapshot")) return false;
  if (!copy_whole(C, &S->fsave, C->fsave, C->fsave.n, &S->bytes) ||
      !copy_whole(C, &S->hcall, C->hcall, C->n, &S->bytes) ||
      !copy_whole(C, &S->status, C->status, C->n, &S->bytes) ||
      !copy_whole(C, &S->counts, C->counts, C->n, &S->bytes) ||
      !copy_whole(C, &S->results, C->results, C->results.n, &S->bytes) ||
      !C->hip_ok(hipStreamSynchronize(C->stream), "snapshot") ||
      !C->hip_ok(hipMemcpy(hc.data(), C->hcall.ptr, size_t(C->n) * 4, hipMemcpyDeviceToHost), "snapshot"))
    return false;
  if (C->staged.calls_on && !C->calls_mirror()) return false;   // (a device-staged vector: fetched now)
  S->susp_h.assign(C->n, 0);
  S->suspended = 0;
  for (uint32_t i = 0; i < C->n; i++)
    if (rpc[i] != 0xFFFFFFFFu && hc[i] == WB_SUSPENDED) {
      S->susp_h[i] = 1;
      S->suspended++;
    }
  S->staged = C->staged;
  S->inv_pc = C->inv_pc;
  S->has_inv = true;
  return true;
}

// Instances that hold pool rows (the caller settled and waited for the stream): the reserved
// layout takes them (hostcall.cpp grow_layout). false, with the message, when it cannot or on
// a device error; the context stays as it was.
bool take_pool_rows(Ctx *C) {
  if (!C->grow_host || !C->pool_used) return true;
  std::vector<uint32_t> pages;
  if (!fetch_slot(C, LS_PAGES, &pages)) return false;
  uint32_t reached = 0;
  for (uint32_t i = 0; i < C->n; i++) reached = std::max(reached, pages[i]);
  if (reached > C->rpages && !grow_layout(C, reached, reached, true)) return false;
  if (reached > C->rpages) {
    C->last_error = "snapshot: instances hold pages past the reserved layout, which cannot grow to take "
                    "them (device memory, MemoryPoolBytes or WB_RELAYOUT=0)";
    return false;
  }
  return true;
}

Snap *create_one(Ctx *C, uint8_t *code, bool inv) {
  DevScope dev(C);
  const wb::Program &P = C->prog;
  *code = kRuntimeError;
  // a Reset that did not wait, or was left to the next launch, is carried out first: the
  // capture must see the reset state
  if (!C->settle() || !C->hip_ok(hipStreamSynchronize(C->stream), "snapshot")) return nullptr;
  // instances that hold pool rows: the reserved layout takes them (hostcall.cpp grow_layout),
  // so that a snapshot never holds a page at or above the rpages it records
  if (!take_pool_rows(C)) return nullptr;
  std::unique_ptr<Snap> S(new Snap());
  S->device = C->device;
  S->n = C->n;
  S->nwaves = C->nwaves;
  S->mlog = C->mlog;
  S->mem_words = C->mem_words;
  S->ls_slots = C->ls_slots;
  S->tab_words = P.mut_tables ? P.tab_words : 0;
  S->tabinfo = P.tabinfo;
  S->xlog = C->xlog;
  S->xwords = C->xwords;
  // memory 0: the rows below every wave's write-mark bound, packed
  std::vector<uint32_t> marks;
  std::vector<uint64_t> off;
  if (!fetch_slot(C, LS_HWM, &marks)) return nullptr;
  const uint32_t mw = P.has_mem ? C->mem_words : 0;
  const uint64_t words = wbs::pack_rows(marks.data(), C->nwaves, C->image_words, mw, &S->rows_h, &off);
  for (uint32_t r : S->rows_h) S->max_tiles = std::max(S->max_tiles, r / wbs::kTile);
  if (!S->mem.alloc(size_t(words) + 4) || !S->rows.upload(S->rows_h, C->stream) || !S->off.upload(off, C->stream)) {
    (void)hipGetLastError();
    C->last_error = "snapshot: no device memory";
    return nullptr;
  }
  S->bytes = (words + 4) * 4 + uint64_t(C->nwaves) * 12;
  SnapMemParams p{};
  p.mem = C->mem.ptr;
  p.snap = S->mem.ptr;
  p.snap_off = S->off.ptr;
  p.snap_rows = S->rows.ptr;
  p.nwaves = C->nwaves;
  p.mem_words = mw;
  p.ls_slots = C->ls_slots;
  p.image_words = C->image_words;
  p.g_mem = p.g_snap = C->mlog;
  p.chunks = chunks_for(C->nwaves, S->max_tiles);
  if (words && !C->hip_ok(wb_launch_snap_mem(&p, 0, C->stream), "snapshot")) return nullptr;
  // instance state, per-lane tables, memories 1..7 and their sizes: whole
  const size_t nw = C->nwaves;
  if (!copy_whole(C, &S->lstate, C->lstate, nw * C->ls_slots * 64, &S->bytes) ||
      !copy_whole(C, &S->ltab, C->ltab, nw * S->tab_words * 64, &S->bytes) ||
      !copy_whole(C, &S->xmem, C->xmem, P.xmems.empty() ? 0 : nw * 64 * size_t(C->xwords), &S->bytes) ||
      !copy_whole(C, &S->xpages, C->xpages, P.xmems.empty() ? 0 : C->xpages0.size(), &S->bytes) ||
      !C->hip_ok(hipStreamSynchronize(C->stream), "snapshot"))
    return nullptr;
  if (inv && !capture_invocation(C, S.get())) return nullptr;
  S->wasi = C->wasi_lanes;
  S->ctx = C;
  {
    std::lock_guard<std::mutex> g(wbs::g_mu);
    C->snaps.push_back(S.get());
  }
  *code = 0;
  return S.release();
}

void delete_one(Snap *S) {
  {
    std::lock_guard<std::mutex> g(wbs::g_mu);
    if (S->ctx) {
      auto &v = S->ctx->snaps;
      v.erase(std::remove(v.begin(), v.end(), S), v.end());
    }
  }
  for (Snap *s : S->subs)
    if (s) delete_one(s);
  int cur = -1;
  const bool sw = !S->subs.size() && hipGetDevice(&cur) == hipSuccess && cur != S->device &&
                  hipSetDevice(S->device) == hipSuccess;
  delete S;   // (its device buffers)
  if (sw) (void)hipSetDevice(cur);
}

uint8_t rows_launch(Ctx *C, uint32_t *dst, const uint32_t *src, const uint32_t *src_of, uint32_t words_d,
                    uint32_t words_s, uint32_t base_d, uint32_t base_s, uint32_t count, uint32_t g,
                    uint32_t fill, uint32_t ls_fix, bool keep) {
  SnapRowsParams r{};
  r.dst = dst;
  r.src = src;
  r.src_of = src_of;
  r.nwaves = C->nwaves;
  r.words_d = words_d;
  r.words_s = words_s;
  r.base_d = base_d;
  r.base_s = base_s;
  r.count = count;
  r.g = g;
  r.fill = fill;
  r.ls_fix = ls_fix;
  r.keep = keep ? 1 : 0;
  return C->hip_ok(wb_launch_snap_rows(&r, C->stream), "restore") ? 0 : kRuntimeError;
}

// What kept lanes need before a restore changes anything (DESIGN.md "Selective restore"): a
// deferred Reset carried out, the pool rows taken into the reserved layout. false, with the
// message, when that cannot be done; the context stays as it was. Doing it again is harmless.
bool prepare_keep(Ctx *C) {
  DevScope dev(C);
  return C->settle() && C->hip_ok(hipStreamSynchronize(C->stream), "restore") && take_pool_rows(C);
}

const char *const kKeepInvocation =
    "restore: a map that keeps instances cannot go with a snapshot that holds an invocation "
    "(SnapshotCreateSuspended)";

// The plan of a restore through SrcDev, a map on the device (wb_snap_plan_kernel), into
// S->plan_src / S->plan_wave; sum: its summary, read back with one synchronise.
bool device_plan(Ctx *C, const Snap *S, const uint32_t *SrcDev, bool same, uint32_t sum[4]) {
  if ((!S->plan_src.ptr && !S->plan_src.alloc(size_t(C->nwaves) * 64)) ||
      (!S->plan_wave.ptr && !S->plan_wave.alloc(size_t(C->nwaves) * 2)) ||
      (!S->plan_sum.ptr && !S->plan_sum.alloc(4))) {
    (void)hipGetLastError();
    C->last_error = "restore: no device memory";
    return false;
  }
  SnapPlanParams q{};
  q.map = SrcDev;
  q.snap_rows = S->rows.ptr;
  q.plan_src = S->plan_src.ptr;
  q.wave_plan = S->plan_wave.ptr;
  q.summary = S->plan_sum.ptr;
  q.n = C->n;
  q.nwaves = C->nwaves;
  q.same_granule = same ? 1 : 0;
  return C->hip_ok(hipMemsetAsync(S->plan_sum.ptr, 0, 16, C->stream), "restore") &&
         C->hip_ok(wb_launch_snap_plan(&q, C->stream), "restore") &&
         C->hip_ok(hipMemcpyAsync(sum, S->plan_sum.ptr, 16, hipMemcpyDeviceToHost, C->stream), "restore") &&
         C->hip_ok(hipStreamSynchronize(C->stream), "restore");
}

// SrcOf: the map on the host, SrcDev: on the device (at most one; both NULL: every instance
// from itself). selected: an entry may be wbs::kKeep (WasmEdge_BatchSnapshotRestoreSelected).
uint8_t restore_one(Ctx *C, const Snap *S, const uint32_t *SrcOf, const uint32_t *SrcDev, bool selected,
                    uint32_t *Restored, double *KernelSeconds) {
  const wb::Program &P = C->prog;
  bool any_keep = false, gather = false;
  uint32_t restored = C->n;
  if (SrcOf)
    for (uint32_t i = 0; i < C->n; i++) {
      if (selected && SrcOf[i] == wbs::kKeep) any_keep = true;
      else if (SrcOf[i] >= C->n)
        return C->fail(kWrongVMWorkflow, selected ? "restore: SrcOf holds an entry that is neither KEEP nor below NumInstances"
                                                  : "restore: SrcOf names an instance past NumInstances");
    }
  if (any_keep && S->has_inv) return C->fail(kWrongVMWorkflow, kKeepInvocation);
  // the layout now against the one recorded: the reserved layout and the tables only grow
  bool fits = S->n == C->n && S->ls_slots == C->ls_slots && S->xwords == C->xwords && S->xlog == C->xlog &&
              S->tabinfo.size() == P.tabinfo.size() && (!P.has_mem || S->mem_words <= C->mem_words) && !C->mem_fresh;
  for (size_t t = 0; fits && S->tab_words && 2 * t + 1 < S->tabinfo.size(); t++)
    fits = S->tabinfo[2 * t + 1] <= P.tabinfo[2 * t + 1];
  if (!fits) return C->fail(kRuntimeError, "restore: the context's layout cannot hold the snapshot");
  DevScope dev(C);
  // A map on the device. The host-side WASI lane state and the host mirrors of an invocation
  // (call_func, call_status, susp_h) need the map on the host: it is read back once and takes
  // the host path. Otherwise the device plans, and nothing that changes state is launched
  // before its summary is here.
  if (SrcDev && (S->has_inv || !S->wasi.empty())) {
    std::vector<uint32_t> map(C->n);
    if (!C->hip_ok(hipMemcpy(map.data(), SrcDev, size_t(C->n) * 4, hipMemcpyDeviceToHost), "restore"))
      return kRuntimeError;
    return restore_one(C, S, map.data(), nullptr, true, Restored, KernelSeconds);
  }
  bool same = S->mlog == C->mlog;
  if (SrcDev) {
    uint32_t sum[4] = {0, 0, 0, 0};
    if (!device_plan(C, S, SrcDev, same, sum)) return kRuntimeError;
    if (sum[0])
      return C->fail(kWrongVMWorkflow, "restore: SrcOf holds an entry that is neither KEEP nor below NumInstances "
                                       "(instance " + std::to_string(~sum[0]) + ")");
    any_keep = sum[1] != 0;
    gather = sum[2] != 0;
    restored = sum[3];
  }
  // Kept lanes (DESIGN.md "Selective restore"). A Reset left to the next launch is carried
  // out first, as a capture does: cancelled, the kept lanes would miss it. And a kept lane may
  // hold pages past the reserved layout: the layout takes the pool rows as at a capture, so
  // that pool_reset below has nothing of a kept lane to lose; when it cannot, nothing changed.
  if (any_keep && !prepare_keep(C)) return kRuntimeError;   // (the granule is a Reset's to change: `same` holds)
  const uint32_t mw = P.has_mem ? C->mem_words : 0;
  const bool mapped = SrcOf || SrcDev;
  const bool planned = mapped || !same;
  if (planned && !SrcDev) {
    wbs::plan_restore(SrcOf, C->n, C->nwaves, S->rows_h.data(), same, &S->plan);
    gather = !S->plan.identity;
    restored = S->plan.restored;
  }
  // a suspended invocation: the call stack deep enough for the rows its sources hold (a Reset
  // since the capture returned it to its first depth) and the result rows at the captured
  // stride, before anything of the context's state changes
  if (S->has_inv) {
    const uint32_t need = wbs::plan_stack(SrcOf ? S->plan.src.data() : nullptr, C->nwaves, S->gs_rows_h.data(), &S->gs_plan);
    if (need > C->gs_depth && !grow_stack(C, S->gs_depth))
      return C->fail(kRuntimeError, "restore: the call stack cannot grow back to the depth of the capture "
                                    "(device memory, CallStackMaxBytes)");
    const size_t rn = size_t(C->n) * (S->staged.result_cells ? S->staged.result_cells : 1);
    if ((SrcOf && !S->gs_plan_d.ptr && !S->gs_plan_d.alloc(S->gs_plan.size())) ||
        ((C->results.n != rn || !C->results.ptr) && !C->results.alloc(rn))) {
      (void)hipGetLastError();
      return C->fail(kRuntimeError, "restore: no device memory");
    }
    if (SrcOf && !C->hip_ok(hipMemcpyAsync(S->gs_plan_d.ptr, S->gs_plan.data(), S->gs_plan.size() * 4,
                                           hipMemcpyHostToDevice, C->stream), "restore"))
      return kRuntimeError;
  }
  // A Reset left to the next launch is cancelled, not carried out: the restore re-initialises
  // every row below the waves' current bound itself and writes every state slot, and that
  // launch would otherwise wipe what it restored. A Reset that is queued orders before the
  // restore's kernels on the stream; nothing here reads instance state from the host, so an
  // untimed restore does not wait for it. (With a kept lane it was carried out above.)
  C->reset_deferred = false;
  if (planned && !SrcDev) {
    if ((!S->plan_src.ptr && !S->plan_src.alloc(S->plan.src.size())) ||
        (!S->plan_wave.ptr && !S->plan_wave.alloc(S->plan.wave.size()))) {
      (void)hipGetLastError();
      return C->fail(kRuntimeError, "restore: no device memory");
    }
    if (!C->hip_ok(hipMemcpyAsync(S->plan_src.ptr, S->plan.src.data(), S->plan.src.size() * 4,
                                  hipMemcpyHostToDevice, C->stream), "restore") ||
        !C->hip_ok(hipMemcpyAsync(S->plan_wave.ptr, S->plan.wave.data(), S->plan.wave.size() * 4,
                                  hipMemcpyHostToDevice, C->stream), "restore"))
      return kRuntimeError;
  }
  const uint32_t *src_of = mapped ? S->plan_src.ptr : nullptr;
  (void)hipEventRecord(C->ev0, C->stream);
  // no restored lane needs a pool row (create_one), and the layout took the kept lanes': the
  // context's go back
  if (!pool_reset(C)) return kRuntimeError;
  SnapMemParams p{};
  p.mem = C->mem.ptr;
  p.snap = S->mem.ptr;
  p.snap_off = S->off.ptr;
  p.snap_rows = S->rows.ptr;
  p.lstate = C->lstate.ptr;
  p.image = C->image.ptr;
  p.src = S->plan_src.ptr;
  p.wave_plan = S->plan_wave.ptr;
  p.nwaves = C->nwaves;
  p.mem_words = mw;
  p.ls_slots = C->ls_slots;
  p.image_words = C->image_words;
  p.g_mem = C->mlog;
  p.g_snap = S->mlog;
  // (the current bounds are the device's to read; the snapshot's rows size the grid)
  p.chunks = chunks_for(C->nwaves, S->max_tiles);
  if (!C->hip_ok(wb_launch_snap_mem(&p, (planned && gather ? 2 : 1) + (any_keep ? 2 : 0), C->stream), "restore"))
    return kRuntimeError;
  // the state slots after memory 0 (whose kernel read the current marks), "not parked"
  // (a suspended invocation keeps its resume points: LS_RPC / LS_GSP / LS_HBASE as captured)
  uint8_t e = rows_launch(C, C->lstate.ptr, S->lstate.ptr, src_of, C->ls_slots, S->ls_slots, 0, 0, C->ls_slots, 0, 0,
                          S->has_inv ? 0 : 1, any_keep);
  // per-lane tables, table by table: the capacities may have widened since (widen_tables);
  // the slots past the captured capacity are null
  for (uint32_t t = 0; !e && S->tab_words && t < P.ntables; t++) {
    const uint32_t fs = S->tabinfo[2 * t], cs = S->tabinfo[2 * t + 1], fc = P.tabinfo[2 * t], cc = P.tabinfo[2 * t + 1];
    e = rows_launch(C, C->ltab.ptr, S->ltab.ptr, src_of, P.tab_words, S->tab_words, fc, fs, cs, 0, 0, 0, any_keep);
    if (!e && cc > cs)   // (a kept lane's widened table keeps its slots: the map goes along)
      e = rows_launch(C, C->ltab.ptr, nullptr, any_keep ? src_of : nullptr, P.tab_words, 0, fc + cs, 0, cc - cs, 0,
                      0xFFFFFFFFu, 0, any_keep);
  }
  if (!e && !P.xmems.empty() && C->xwords)
    e = rows_launch(C, C->xmem.ptr, S->xmem.ptr, src_of, C->xwords, S->xwords, 0, 0, C->xwords, C->xlog, 0, 0,
                    any_keep);
  const size_t xs = size_t(C->nwaves) * 64;
  for (size_t k = 0; !e && k < P.xmems.size(); k++)
    e = rows_launch(C, C->xpages.ptr + k * xs, S->xpages.ptr + k * xs, src_of, 1, 1, 0, 0, 1, 0, 0, 0, any_keep);
  // the suspended invocation: frame-save rows, the call-stack rows of the sources, and status,
  // count, hcall and result row of every instance
  if (!e && S->has_inv) {
    const uint32_t fw = uint32_t(P.total_cells() ? P.total_cells() : 1) + C->gs_lds;
    e = rows_launch(C, C->fsave.ptr, S->fsave.ptr, src_of, fw, fw, 0, 0, fw, 0, 0, 0, false);
    SnapStackParams k{};
    k.gstack = C->gstack.ptr;
    k.snap = S->gs.ptr;
    k.snap_off = S->gs_off.ptr;
    k.snap_rows = S->gs_rows.ptr;
    k.src = S->plan_src.ptr;
    k.wave_plan = S->gs_plan_d.ptr;
    k.snap_words = S->gs_words;
    k.nwaves = C->nwaves;
    k.gs_depth = C->gs_depth;
    k.chunks = stack_chunks(C->nwaves, S->gs_rows_h);
    if (!e && !C->hip_ok(wb_launch_snap_stack(&k, SrcOf ? 2 : 1, C->stream), "restore")) e = kRuntimeError;
    SnapInstParams q{};
    q.status_d = C->status.ptr;
    q.status_s = S->status.ptr;
    q.counts_d = C->counts.ptr;
    q.counts_s = S->counts.ptr;
    q.hcall_d = C->hcall.ptr;
    q.hcall_s = S->hcall.ptr;
    q.results_d = C->results.ptr;
    q.results_s = S->results.ptr;
    q.src_of = src_of;
    q.n = C->n;
    q.result_cells = S->staged.result_cells;
    if (!e && !C->hip_ok(wb_launch_snap_inst(&q, C->stream), "restore")) e = kRuntimeError;
  }
  if (e) return e;
  (void)hipEventRecord(C->ev1, C->stream);
  // the host-side WASI lane state through SrcOf; `index` and an instance's own args stay, and
  // a kept instance keeps its lane
  if (!S->wasi.empty() && S->wasi.size() == C->wasi_lanes.size()) {
    std::vector<wbw::Lane> lanes(C->n);
    for (uint32_t i = 0; i < C->n; i++) {
      lanes[i] = SrcOf && SrcOf[i] == wbs::kKeep ? C->wasi_lanes[i] : S->wasi[SrcOf ? SrcOf[i] : i];
      lanes[i].index = C->wasi_lanes[i].index;
      lanes[i].own_args = C->wasi_lanes[i].own_args;
      lanes[i].args = C->wasi_lanes[i].args;
    }
    C->wasi_lanes.swap(lanes);
  }
  C->ran = false;
  C->end_invocation();       // (a snapshot without frames: a suspended invocation ends here)
  C->reset_pending = true;   // host accessors settle() before touching instance state
  if (S->has_inv) {
    // the invocation's descriptor, the per-instance fields through SrcOf; BatchResume
    // continues it and BatchResults reads the rows as they stood (it does not settle: wait)
    // (the arguments on the device stay the staged ones, so their fingerprint stays too: a
    // Run needs them staged again unless they are what the invocation ran on)
    const uint64_t fp = C->staged.args_fp;
    C->restage = SrcOf || !C->staged.same_run(S->staged);
    C->staged = S->staged;
    C->staged.args_fp = fp;
    C->suspended = 0;
    for (uint32_t i = 0; i < C->n; i++) {
      const uint32_t s = SrcOf ? SrcOf[i] : i;
      C->suspended += S->susp_h[s];
      if (S->staged.calls_on && SrcOf) {
        C->staged.call_func[i] = S->staged.call_func[s];
        C->staged.call_status[i] = S->staged.call_status[s];
      }
    }
    // (calls_io: the host copy is the current one, CallsResultsDevice uploads it on first need)
    C->call_host_ok = true;
    C->call_dev_ok = false;
    C->calls_shape();
    C->inv_pc = S->inv_pc;
    C->inv_live = true;
    C->ran = true;
    C->reset_pending = false;
    if (!C->hip_ok(hipStreamSynchronize(C->stream), "restore")) {
      C->end_invocation();
      C->ran = false;
      return kRuntimeError;
    }
  }
  if (KernelSeconds) {
    C->reset_pending = false;
    if (!C->hip_ok(hipStreamSynchronize(C->stream), "restore")) return kRuntimeError;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, C->ev0, C->ev1);
    *KernelSeconds = ms * 1e-3;
  }
  if (Restored) *Restored = restored;
  return 0;
}

}  // namespace

static Snap *create(Ctx *C, WasmEdge_Result *Res, bool inv) {
  if (!C) {
    if (Res) *Res = R(kWrongVMWorkflow);
    return nullptr;
  }
  // an invocation capture needs a live invocation: a completed Run / Resume of a Resumable
  // context that nothing has ended since (on every shard: they end together)
  bool live = C->shards.empty() ? C->conf.Resumable && C->inv_live : true;
  for (Ctx *s : C->shards) live = live && (!s || (s->conf.Resumable && s->inv_live));
  if (inv && !live) {
    C->last_error = C->conf.Resumable ? "SnapshotCreateSuspended: no live invocation (BatchRun / BatchResume first)"
                                      : "SnapshotCreateSuspended: the context is not Resumable";
    if (Res) *Res = R(kWrongVMWorkflow);
    return nullptr;
  }
  uint8_t code = 0;
  Snap *S = nullptr;
  if (C->shards.empty()) {
    S = create_one(C, &code, inv);
  } else {   // one sub-snapshot per shard
    S = new Snap();
    S->n = C->n;
    S->subs.assign(C->shards.size(), nullptr);
    for (size_t g = 0; g < C->shards.size() && !code; g++) {
      if (!C->shards[g]) continue;
      S->subs[g] = create_one(C->shards[g], &code, inv);
      if (code) C->last_error = C->shards[g]->last_error;
      else S->bytes += S->subs[g]->bytes;
      if (!code) S->suspended += S->subs[g]->suspended;
    }
    if (code) {
      delete_one(S);
      S = nullptr;
    } else {
      S->has_inv = inv;
      S->ctx = C;
      std::lock_guard<std::mutex> g(wbs::g_mu);
      C->snaps.push_back(S);
    }
  }
  if (Res) *Res = R(code);
  return S;
}

extern "C" {

WasmEdge_BatchSnapshot *WasmEdge_BatchSnapshotCreate(WasmEdge_BatchContext *C, WasmEdge_Result *Res) {
  return create(C, Res, false);
}

WasmEdge_BatchSnapshot *WasmEdge_BatchSnapshotCreateSuspended(WasmEdge_BatchContext *C, WasmEdge_Result *Res) {
  return create(C, Res, true);
}

uint32_t WasmEdge_BatchSnapshotGetSuspendedCount(const WasmEdge_BatchSnapshot *S) {
  return S && S->has_inv ? S->suspended : 0;
}

WasmEdge_Result WasmEdge_BatchSnapshotRestore(WasmEdge_BatchContext *C, const WasmEdge_BatchSnapshot *S,
                                              const uint32_t *SrcOf, double *KernelSeconds) {
  if (!C || !S) return R(kWrongVMWorkflow);
  if (S->ctx != C) return R(C->fail(kWrongVMWorkflow, "restore: the snapshot was taken from another context"));
  if (C->shards.empty()) return R(restore_one(C, S, SrcOf, nullptr, false, nullptr, KernelSeconds));
  if (SrcOf) {
    for (uint32_t i = 0; i < C->n; i++)
      if (SrcOf[i] >= C->n) return R(C->fail(kWrongVMWorkflow, "restore: SrcOf names an instance past NumInstances"));
    return R(C->fail(kRuntimeError, "restore: SrcOf on a multi-device context (rows cannot cross devices); "
                                    "pass NULL to restore every instance from itself"));
  }
  double secs = 0;
  for (size_t g = 0; g < C->shards.size(); g++) {
    if (!C->shards[g]) continue;
    double t = 0;
    const uint8_t e = restore_one(C->shards[g], S->subs[g], nullptr, nullptr, false, nullptr, KernelSeconds ? &t : nullptr);
    if (e) {
      C->last_error = C->shards[g]->last_error;
      return R(e);
    }
    secs = std::max(secs, t);
  }
  if (KernelSeconds) *KernelSeconds = secs;
  return R(0);
}

WasmEdge_Result WasmEdge_BatchSnapshotRestoreSelected(WasmEdge_BatchContext *C, const WasmEdge_BatchSnapshot *S,
                                                      const uint32_t *SrcOf, uint32_t *NumRestored,
                                                      double *KernelSeconds) {
  if (!C || !S || !SrcOf) return R(kWrongVMWorkflow);
  if (S->ctx != C) return R(C->fail(kWrongVMWorkflow, "restore: the snapshot was taken from another context"));
  if (C->shards.empty()) return R(restore_one(C, S, SrcOf, nullptr, true, NumRestored, KernelSeconds));
  // shards: legal when nothing crosses a device -- every entry KEEP or the instance itself;
  // the map is sliced by the placement
  bool keep = false, local = true;
  for (uint32_t i = 0; i < C->n; i++) {
    if (SrcOf[i] == wbs::kKeep) keep = true;
    else if (SrcOf[i] >= C->n)
      return R(C->fail(kWrongVMWorkflow, "restore: SrcOf holds an entry that is neither KEEP nor below NumInstances"));
    else local = local && SrcOf[i] == i;
  }
  if (keep && S->has_inv) return R(C->fail(kWrongVMWorkflow, kKeepInvocation));
  if (!local)
    return R(C->fail(kRuntimeError, "restore: SrcOf on a multi-device context (rows cannot cross devices); "
                                    "every entry must be KEEP or the instance itself"));
  std::vector<std::vector<uint32_t>> maps(C->shards.size());
  for (size_t g = 0; g < C->shards.size(); g++)
    if (C->shards[g]) maps[g].resize(C->shards[g]->n);
  for (uint32_t i = 0; i < C->n; i++) {
    Ctx *sh = nullptr;
    uint32_t at = 0;
    if (!wbm::route(C, i, &sh, &at)) return R(C->fail(kRuntimeError, "restore: an instance without a shard"));
    for (size_t g = 0; g < C->shards.size(); g++)
      if (C->shards[g] == sh) maps[g][at] = SrcOf[i] == wbs::kKeep ? wbs::kKeep : at;
  }
  // what can fail for want of room (a kept lane's pool rows) on every shard before the first
  // restore, so that such a failure leaves all shards as they were
  for (size_t g = 0; keep && g < C->shards.size(); g++)
    if (C->shards[g] && !prepare_keep(C->shards[g])) {
      C->last_error = C->shards[g]->last_error;
      return R(kRuntimeError);
    }
  double secs = 0;
  uint32_t total = 0;
  for (size_t g = 0; g < C->shards.size(); g++) {
    if (!C->shards[g]) continue;
    double t = 0;
    uint32_t r = 0;
    const uint8_t e = restore_one(C->shards[g], S->subs[g], maps[g].data(), nullptr, true, &r, KernelSeconds ? &t : nullptr);
    if (e) {
      C->last_error = C->shards[g]->last_error;
      return R(e);
    }
    secs = std::max(secs, t);
    total += r;
  }
  if (KernelSeconds) *KernelSeconds = secs;
  if (NumRestored) *NumRestored = total;
  return R(0);
}

WasmEdge_Result WasmEdge_BatchSnapshotRestoreSelectedDevice(WasmEdge_BatchContext *C, const WasmEdge_BatchSnapshot *S,
                                                            const uint32_t *SrcOfDevice, uint32_t *NumRestored,
                                                            double *KernelSeconds) {
  if (!C || !S || !SrcOfDevice) return R(kWrongVMWorkflow);
  if (S->ctx != C) return R(C->fail(kWrongVMWorkflow, "restore: the snapshot was taken from another context"));
  if (!C->shards.empty())
    return R(C->fail(kRuntimeError, "restore: a device map on a multi-device context (use the host entry)"));
  {   // NumInstances words there, as far as this HIP runtime knows the allocation
    DevScope dev(C);
    if (!device_rows_ok(C, SrcOfDevice, 4, 4, "restore: the map is not a buffer on the context's device",
                        "restore: the device map is smaller than NumInstances words"))
      return R(kRuntimeError);
  }
  return R(restore_one(C, S, nullptr, SrcOfDevice, true, NumRestored, KernelSeconds));
}

uint64_t WasmEdge_BatchSnapshotGetBytes(const WasmEdge_BatchSnapshot *S) { return S ? S->bytes : 0; }

void WasmEdge_BatchSnapshotDelete(WasmEdge_BatchSnapshot *S) {
  if (S) delete_one(S);
}

}  // extern "C"
