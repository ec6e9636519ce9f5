// staging.cpp -- what a Run works on and what it leaves behind: BatchSetArgs / SetCalls and
// their device-resident forms stage it (a wbh::Staging and the buffers that go with it),
// BatchGetReturnLens / Results and their device-resident forms read it back. How a
// signature's values lie in cells, slots and tables is sig_layout.h's; batch_api.cpp launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "args_io.h"
#include "batch_ctx.h"
#include "multi.h"

using namespace wbh;
using Ctx = WasmEdge_BatchContext;

bool wbh::device_rows_ok(Ctx *C, const void *Buf, uint64_t row, uint64_t stride, const char *not_device,
                         const char *too_small) {
  if (!Buf || !row || !C->n) return true;
  hipPointerAttribute_t at{};
  void *base = nullptr;
  size_t size = 0;
  if (hipPointerGetAttributes(&at, Buf) != hipSuccess || at.type == hipMemoryTypeUnregistered) {
    (void)hipGetLastError();
    return true;
  }
  if (at.type != hipMemoryTypeDevice || at.device != C->device ||
      hipMemGetAddressRange(&base, &size, const_cast<void *>(Buf)) != hipSuccess) {
    (void)hipGetLastError();
    C->fail(kRuntimeError, not_device);
    return false;
  }
  const uint64_t room = uint64_t(size) - uint64_t(static_cast<const uint8_t *>(Buf) - static_cast<uint8_t *>(base));
  if (room < row || (C->n > 1 && stride > (room - row) / (C->n - 1))) {
    C->fail(kRuntimeError, too_small);
    return false;
  }
  return true;
}

namespace {

std::string str(const WasmEdge_String &s) { return std::string(s.Buf ? s.Buf : "", s.Length); }

// the table on the device, uploaded when it differs from the one there (`host`)
bool upload_map(Ctx *C, DevBuf<uint32_t> &dev, std::vector<uint32_t> &host, std::vector<uint32_t> &map) {
  if (dev.ptr && host == map) return true;
  host.clear();   // (nothing valid there until the copy is queued)
  if (dev.n < map.size() && !dev.alloc(map.size())) {
    (void)hipGetLastError();
    C->fail(kRuntimeError, "device allocation failed");
    return false;
  }
  host.swap(map);   // (the copy's source lives as long as the context)
  return C->hip_ok(hipMemcpyAsync(dev.ptr, host.data(), host.size() * 4, hipMemcpyHostToDevice, C->stream),
                   "signature table upload");
}
template <typename T>
void swap_bufs(DevBuf<T> &a, DevBuf<T> &b) {
  std::swap(a.ptr, b.ptr);
  std::swap(a.n, b.n);
}
// (a buffer stays when its size does: a caller passing new arguments every run pays no device
// allocation, and the kernel reads the same pages)
template <typename T>
bool sized(DevBuf<T> &b, size_t count) {
  return (b.ptr && b.n == count) || b.alloc(count);
}
// elements of an [n][cells] buffer (never empty)
size_t rows(const Ctx *C, uint32_t cells) { return size_t(C->n) * (cells ? cells : 1); }

uint64_t fold(uint64_t fp, const std::vector<uint32_t> &words) {
  for (uint32_t c : words) fp = (fp ^ c) * 0x100000001B3ull + (fp >> 29);
  return fp;
}

// an externref's cell: the value interned (batch_ctx.h xref_in); false: the intern table is full.
// Kept out of line so that put_value stays small enough to be inlined into the packing loops
// (as a call per value SetArgs took a quarter longer at 65,536 x 8 values).
__attribute__((noinline)) bool put_xref(Ctx *C, uint128_t v, uint32_t *at) {
  bool full = false;
  *at = C->xref_in(v, &full);
  if (full) C->fail(kRuntimeError, "externref intern table full (2^31 - 1 values)");
  return !full;
}
// one host value's cells at `at`, which moves past them
__attribute__((always_inline)) inline bool put_value(Ctx *C, uint8_t ty, const WasmEdge_Value &v, uint32_t *&at) {
  if (ty == wb::EXTERNREF) return put_xref(C, v.Value, at++);
  at += wb::to_cells(ty, v.Value, at);
  return true;
}

// the export a uniform staging names (executor.cpp:88-100: the parameter count must match,
// the types are the caller's to compare); nullptr: *e
const wb::FuncType *uniform_export(Ctx *C, const WasmEdge_String &FuncName, uint32_t ParamLen, int *f, uint8_t *e) {
  const std::string name = str(FuncName);
  *f = wb::find_export(C->prog, name);
  if (*f < 0) *e = C->fail(kFuncNotFound, "function '" + name + "' not found");
  else if (ParamLen != C->prog.types[C->prog.funcs[*f].type].params.size())
    *e = C->fail(kFuncSigMismatch, "parameter count mismatch");
  else return &C->prog.types[C->prog.funcs[*f].type];
  return nullptr;
}

// the new staging takes effect (a suspended invocation cannot continue)
WasmEdge_Result commit(Ctx *C, Staging &s) {
  C->staged = std::move(s);
  C->restage = false;
  C->end_invocation();
  return R(0);
}
// ... one function for every instance
WasmEdge_Result commit_uniform(Ctx *C, int f, const wb::FuncType &t, const wb::SigLayout &L, uint64_t fp) {
  Staging s;
  s.func = f;
  s.param_cells = L.param_cells;
  s.result_cells = L.result_cells;
  s.result_types = t.results;
  s.args_fp = fp;
  return commit(C, s);
}
// ... per-instance calls, their vector current on the host or on the device (calls_io: the
// other side's copy is stale)
WasmEdge_Result commit_calls(Ctx *C, Staging &s, bool host) {
  s.calls_on = true;
  commit(C, s);
  C->call_host_ok = host;
  C->call_dev_ok = !host;
  if (host) C->calls_shape();
  return R(0);
}

// what both device result calls end with: statuses and counts device to device, one synchronise
WasmEdge_Result finish_device_results(Ctx *C, uint8_t *PerInstance, uint64_t *InstrCounts) {
  if (PerInstance && !C->hip_ok(hipMemcpyAsync(PerInstance, C->status.ptr, C->n, hipMemcpyDeviceToDevice, C->stream), "status"))
    return R(kRuntimeError);
  if (InstrCounts && !C->hip_ok(hipMemcpyAsync(InstrCounts, C->counts.ptr, size_t(C->n) * 8, hipMemcpyDeviceToDevice,
                                               C->stream), "counts"))
    return R(kRuntimeError);
  if (!C->hip_ok(hipStreamSynchronize(C->stream), "results unpack")) return R(kRuntimeError);
  return R(0);
}

}  // namespace

extern "C" {

WasmEdge_Result WasmEdge_BatchSetArgs(WasmEdge_BatchContext *C, const WasmEdge_String FuncName,
                                      const WasmEdge_Value *Params, const uint32_t ParamLen) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty()) return wbm::set_args(C, FuncName, Params, ParamLen);
  DevScope dev(C);
  int f;
  uint8_t e = 0;
  const wb::FuncType *t = uniform_export(C, FuncName, ParamLen, &f, &e);
  if (!t) return R(e);
  const wb::SigLayout L = wb::layout_of(*t);
  std::vector<uint32_t> cells(rows(C, L.param_cells));
  uint32_t *at = cells.data();
  for (uint32_t i = 0; i < C->n; i++)
    for (uint32_t k = 0; k < ParamLen; k++) {
      const WasmEdge_Value &v = Params[size_t(i) * ParamLen + k];
      if (uint8_t(v.Type) != t->params[k]) return R(C->fail(kFuncSigMismatch, "parameter type mismatch"));
      if (!put_value(C, t->params[k], v, at)) return R(kRuntimeError);
    }
  if (!sized(C->params, cells.size()) || !sized(C->results, rows(C, L.result_cells)))
    return R(C->fail(kRuntimeError, "device allocation failed"));
  if (!C->hip_ok(hipMemcpyAsync(C->params.ptr, cells.data(), cells.size() * 4,
                                hipMemcpyHostToDevice, C->stream), "params upload"))
    return R(kRuntimeError);
  if (!C->hip_ok(hipStreamSynchronize(C->stream), "params upload")) return R(kRuntimeError);
  // fingerprint of the arguments (the longest-first wave order is reused only on equal ones)
  return commit_uniform(C, f, *t, L, fold(0x9E3779B97F4A7C15ull ^ uint64_t(f), cells));
}

// Per-instance calls: N independent VMExecute calls (vm.cpp:287-308 resolves each name,
// executor.cpp:88-100 checks each signature), so an unknown name or a mismatch is that
// instance's outcome, not the call's. Everything is checked and packed before anything of
// the context changes: a failed call leaves the previous staging as it was.
WasmEdge_Result WasmEdge_BatchSetCalls(WasmEdge_BatchContext *C, const WasmEdge_String *FuncNames,
                                       const uint32_t NumFuncs, const uint32_t *FuncOf,
                                       const WasmEdge_Value *Params, const uint32_t ParamStride,
                                       const uint32_t *ParamLens) {
  if (!C) return R(kWrongVMWorkflow);
  if (!FuncOf || (NumFuncs && !FuncNames)) return R(C->fail(kWrongVMWorkflow, "BatchSetCalls: null FuncOf / FuncNames"));
  for (uint32_t i = 0; i < C->n; i++)
    if (FuncOf[i] != WASMEDGE_BATCH_NO_CALL && FuncOf[i] >= NumFuncs)
      return R(C->fail(kWrongVMWorkflow, "BatchSetCalls: FuncOf[" + std::to_string(i) + "] names no function"));
  if (!C->shards.empty()) return wbm::set_calls(C, FuncNames, NumFuncs, FuncOf, Params, ParamStride, ParamLens);
  DevScope dev(C);
  const wb::Program &P = C->prog;
  std::vector<int> fidx(NumFuncs, -1);
  std::vector<wb::SigLayout> lay(NumFuncs);
  for (uint32_t j = 0; j < NumFuncs; j++) {
    fidx[j] = wb::find_export(P, str(FuncNames[j]));
    if (fidx[j] >= 0) lay[j] = wb::layout_of(P.types[P.funcs[fidx[j]].type]);
  }
  // each instance's function, or the status it sits the run out with
  Staging s;
  s.call_func.assign(C->n, -1);
  s.call_status.assign(C->n, 0);
  for (uint32_t i = 0; i < C->n; i++) {
    const uint32_t j = FuncOf[i];
    if (j == WASMEDGE_BATCH_NO_CALL) continue;
    if (fidx[j] < 0) { s.call_status[i] = kFuncNotFound; continue; }
    const wb::FuncType &t = P.types[P.funcs[fidx[j]].type];
    const uint32_t len = ParamLens ? ParamLens[i] : ParamStride;
    bool ok = len == t.params.size() && len <= ParamStride && (len == 0 || Params);
    for (uint32_t k = 0; ok && k < len; k++) ok = uint8_t(Params[size_t(i) * ParamStride + k].Type) == t.params[k];
    if (!ok) { s.call_status[i] = kFuncSigMismatch; continue; }
    s.call_func[i] = fidx[j];
    s.param_cells = std::max(s.param_cells, lay[j].param_cells);
    s.result_cells = std::max(s.result_cells, lay[j].result_cells);
    s.calls_import |= P.funcs[fidx[j]].imported;
  }
  const uint32_t pc = s.param_cells;
  std::vector<uint32_t> cells(rows(C, pc)), tab(size_t(C->n) * 2);
  for (uint32_t i = 0; i < C->n; i++) {
    tab[2 * i] = WB_CALL_SKIP | s.call_status[i];
    tab[2 * i + 1] = 0;
    if (s.call_func[i] < 0) continue;
    const wb::FuncInfo &F = P.funcs[s.call_func[i]];
    const wb::FuncType &t = P.types[F.type];
    uint32_t *at = &cells[size_t(i) * pc];
    for (uint32_t k = 0; k < t.params.size(); k++)
      if (!put_value(C, t.params[k], Params[size_t(i) * ParamStride + k], at)) return R(kRuntimeError);
    tab[2 * i] = F.imported ? WB_CALL_SKIP : F.entry_pc;   // (an import: BatchRun refuses)
    tab[2 * i + 1] = uint32_t(at - &cells[size_t(i) * pc]);
  }
  if (!sized(C->params, cells.size()) || !sized(C->results, rows(C, s.result_cells)) ||
      (!C->calls.ptr && !C->calls.alloc(tab.size())))
    return R(C->fail(kRuntimeError, "device allocation failed"));
  if (!C->hip_ok(hipMemcpyAsync(C->params.ptr, cells.data(), cells.size() * 4, hipMemcpyHostToDevice,
                                C->stream), "params upload") ||
      !C->hip_ok(hipMemcpyAsync(C->calls.ptr, tab.data(), tab.size() * 4, hipMemcpyHostToDevice,
                                C->stream), "calls upload") ||
      !C->hip_ok(hipStreamSynchronize(C->stream), "params upload"))
    return R(kRuntimeError);
  // fingerprint of the call vector and the arguments (wave order, layout trial)
  s.args_fp = fold(fold(0xC2B2AE3D27D4EB4Full, tab), cells);
  return commit_calls(C, s, true);
}

WasmEdge_Result WasmEdge_BatchGetReturnLens(WasmEdge_BatchContext *C, uint32_t *ReturnLens) {
  if (!C || !ReturnLens) return R(kWrongVMWorkflow);
  if (!C->shards.empty()) return wbm::return_lens(C, ReturnLens);
  const Staging &s = C->staged;
  if (!s.calls_on && s.func < 0) return R(C->fail(kWrongVMWorkflow, "BatchSetArgs / BatchSetCalls not called"));
  if (s.calls_on && !C->calls_mirror()) return R(kRuntimeError);
  for (uint32_t i = 0; i < C->n; i++)
    ReturnLens[i] = !s.calls_on ? uint32_t(s.result_types.size())
                    : s.call_func[i] < 0 ? 0u
                    : uint32_t(C->prog.types[C->prog.funcs[s.call_func[i]].type].results.size());
  return R(0);
}

WasmEdge_Result WasmEdge_BatchResults(WasmEdge_BatchContext *C, WasmEdge_Value *Returns,
                                      const uint32_t ReturnLen, uint8_t *PerInstance,
                                      uint64_t *InstrCounts) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty()) return wbm::results(C, Returns, ReturnLen, PerInstance, InstrCounts);
  if (!C->ran) return R(C->fail(kWrongVMWorkflow, "BatchRun not called"));
  const Staging &s = C->staged;
  if (s.calls_on && Returns && ReturnLen && !C->calls_mirror()) return R(kRuntimeError);
  std::vector<uint8_t> st(C->n);
  if (!C->hip_ok(hipMemcpy(st.data(), C->status.ptr, C->n, hipMemcpyDeviceToHost), "status"))
    return R(kRuntimeError);
  if (PerInstance) memcpy(PerInstance, st.data(), C->n);
  if (InstrCounts &&
      !C->hip_ok(hipMemcpy(InstrCounts, C->counts.ptr, size_t(C->n) * 8, hipMemcpyDeviceToHost), "counts"))
    return R(kRuntimeError);
  if (Returns && ReturnLen) {
    const uint32_t rc = s.result_cells;
    std::vector<uint32_t> cells(rows(C, rc));
    if (rc && !C->hip_ok(hipMemcpy(cells.data(), C->results.ptr, cells.size() * 4,
                                   hipMemcpyDeviceToHost), "results"))
      return R(kRuntimeError);
    // (per-instance calls: each row carries its own function's result types, and an instance
    // that sat the run out a row of zeroes -- the device wrote nothing there)
    static const std::vector<uint8_t> none;
    for (uint32_t i = 0; i < C->n; i++) {
      const std::vector<uint8_t> &types = !s.calls_on ? s.result_types
                                          : s.call_func[i] < 0 ? none
                                          : C->prog.types[C->prog.funcs[s.call_func[i]].type].results;
      if (s.calls_on)
        for (uint32_t k = uint32_t(types.size()); k < ReturnLen; k++) Returns[size_t(i) * ReturnLen + k] = WasmEdge_Value{};
      const uint32_t *at = &cells[size_t(i) * rc];
      for (uint32_t k = 0; k < types.size() && k < ReturnLen; k++) {
        const uint8_t ty = types[k];
        const uint128_t v = wb::from_cells(ty, at);
        at += wb::cells_of(ty);
        WasmEdge_Value &out = Returns[size_t(i) * ReturnLen + k];
        out.Value = st[i] != 0 ? 0 : ty == wb::EXTERNREF ? C->xref_out(uint32_t(v)) : v;
        out.Type = static_cast<enum WasmEdge_ValType>(ty);
      }
    }
  }
  return R(0);
}

// ---- device-resident arguments and results (args_io.hip; DESIGN.md "Device-resident
// arguments and results") ----------------------------------------------------------------

WasmEdge_Result WasmEdge_BatchSetArgsDevice(WasmEdge_BatchContext *C, const WasmEdge_String FuncName,
                                            const enum WasmEdge_ValType *ParamTypes, const uint32_t ParamLen,
                                            const uint64_t *Slots, const uint64_t Stride) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty())
    return R(C->fail(kRuntimeError, "a device buffer cannot serve a multi-device context: use BatchSetArgs"));
  DevScope dev(C);
  int f;
  uint8_t e = 0;
  const wb::FuncType *t = uniform_export(C, FuncName, ParamLen, &f, &e);
  if (!t) return R(e);
  // executor.cpp:88-100, on the type array: a device row carries no tags
  if (ParamLen && !ParamTypes) return R(C->fail(kWrongVMWorkflow, "BatchSetArgsDevice: null ParamTypes"));
  for (uint32_t k = 0; k < ParamLen; k++)
    if (uint8_t(ParamTypes[k]) != t->params[k]) return R(C->fail(kFuncSigMismatch, "parameter type mismatch"));
  const wb::SigLayout L = wb::layout_of(*t);
  if (L.param_xref || L.result_xref)
    return R(C->fail(kRuntimeError, "BatchSetArgsDevice: externref values are interned on the host: use BatchSetArgs"));
  const uint64_t need = L.param_slots;
  const uint32_t pc = L.param_cells;
  if (need && !Slots) return R(C->fail(kWrongVMWorkflow, "BatchSetArgsDevice: null Slots"));
  if (Stride < need) return R(C->fail(kWrongVMWorkflow, "BatchSetArgsDevice: Stride is smaller than a row"));
  if (need && (uintptr_t(Slots) & 7u)) return R(C->fail(kWrongVMWorkflow, "BatchSetArgsDevice: Slots is not 8-byte aligned"));
  if (need && Stride > (~0ull >> 4)) return R(C->fail(kWrongVMWorkflow, "BatchSetArgsDevice: Stride out of range"));
  if (!device_rows_ok(C, Slots, need * 8, Stride * 8, "BatchSetArgsDevice")) return R(kRuntimeError);
  if (!sized(C->params, rows(C, pc)) || !sized(C->results, rows(C, L.result_cells)) ||
      (!C->args_sum.ptr && !C->args_sum.alloc(1)))
    return R(C->fail(kRuntimeError, "device allocation failed"));
  C->args_sum_h = 0;
  if (pc) {
    std::vector<uint32_t> map = wb::pack_map(t->params);
    if (!upload_map(C, C->pack_map, C->pack_map_h, map)) return R(kRuntimeError);
    ArgsPackParams p{};
    p.slots = Slots;
    p.word_of = C->pack_map.ptr;
    p.params = C->params.ptr;
    p.fp = C->args_sum.ptr;
    p.stride = Stride;
    p.n = C->n;
    p.cells = pc;
    if (!C->hip_ok(hipMemsetAsync(C->args_sum.ptr, 0, 8, C->stream), "fingerprint") ||
        !C->hip_ok(wb_launch_args_pack(&p, C->stream), "args pack") ||
        !C->hip_ok(hipMemcpyAsync(&C->args_sum_h, C->args_sum.ptr, 8, hipMemcpyDeviceToHost, C->stream), "fingerprint"))
      return R(kRuntimeError);
  }
  if (!C->hip_ok(hipStreamSynchronize(C->stream), "args pack")) return R(kRuntimeError);
  // the function and the cells' order-independent sum (args_io.h): equal for equal device
  // arguments, not the value BatchSetArgs gives the same arguments
  return commit_uniform(C, f, *t, L, args_fp_mix(~uint64_t(f), 0xA5A5A5A5u) + C->args_sum_h);
}

WasmEdge_Result WasmEdge_BatchResultsDevice(WasmEdge_BatchContext *C, uint64_t *Slots, const uint32_t ReturnLen,
                                            const uint64_t Stride, uint8_t *PerInstance, uint64_t *InstrCounts) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty())
    return R(C->fail(kRuntimeError, "a device buffer cannot serve a multi-device context: use BatchResults"));
  const Staging &s = C->staged;
  if (s.calls_on)
    return R(C->fail(kWrongVMWorkflow, "BatchResultsDevice: per-instance calls have no device rows: use BatchResults"));
  if (!C->ran) return R(C->fail(kWrongVMWorkflow, "BatchRun not called"));
  DevScope dev(C);
  // word w of the written part of a row is result cell map[w] (or zero)
  const uint32_t len = Slots ? ReturnLen : 0;
  for (uint32_t k = 0; k < len && k < s.result_types.size(); k++)
    if (s.result_types[k] == wb::EXTERNREF)
      return R(C->fail(kRuntimeError, "BatchResultsDevice: externref values are interned on the host: use BatchResults"));
  std::vector<uint32_t> map = wb::unpack_map(s.result_types, len);
  const uint64_t need = map.size() / 2;
  if (Stride < need) return R(C->fail(kWrongVMWorkflow, "BatchResultsDevice: Stride is smaller than a row"));
  if (need && (uintptr_t(Slots) & 7u)) return R(C->fail(kWrongVMWorkflow, "BatchResultsDevice: Slots is not 8-byte aligned"));
  if (need && Stride > (~0ull >> 4)) return R(C->fail(kWrongVMWorkflow, "BatchResultsDevice: Stride out of range"));
  if (InstrCounts && (uintptr_t(InstrCounts) & 7u))
    return R(C->fail(kWrongVMWorkflow, "BatchResultsDevice: InstrCounts is not 8-byte aligned"));
  if (!device_rows_ok(C, Slots, need * 8, Stride * 8, "BatchResultsDevice") ||
      !device_rows_ok(C, PerInstance, 1, 1, "BatchResultsDevice") ||
      !device_rows_ok(C, InstrCounts, 8, 8, "BatchResultsDevice"))
    return R(kRuntimeError);
  // (every launch and host-import round of the run has ended: launch_once waits for its
  // kernel, a restore of a suspended invocation for its own)
  if (need) {
    const uint32_t words = uint32_t(map.size());
    if (!upload_map(C, C->unpack_map, C->unpack_map_h, map)) return R(kRuntimeError);
    ArgsUnpackParams p{};
    p.results = C->results.ptr;
    p.status = C->status.ptr;
    p.cell_of = C->unpack_map.ptr;
    p.slots = Slots;
    p.stride = Stride;
    p.n = C->n;
    p.cells = s.result_cells;
    p.words = words;
    if (!C->hip_ok(wb_launch_args_unpack(&p, C->stream), "results unpack")) return R(kRuntimeError);
  }
  return finish_device_results(C, PerInstance, InstrCounts);
}

// ---- device-resident per-instance calls (calls_io.hip; DESIGN.md "Device-resident
// per-instance calls") -------------------------------------------------------------------

// BatchSetCalls from a device FuncOf and device slot rows. The host resolves the NumFuncs
// names into a table; one kernel turns FuncOf and the rows into the call table, the cells and
// call_fn in the spare buffers and reduces the fingerprint, the lowest invalid FuncOf index and
// the "an import is called" flag into 16 bytes, read back with the call's one synchronise. A
// valid vector swaps the spare buffers in; an invalid one leaves the live staging as it was.
WasmEdge_Result WasmEdge_BatchSetCallsDevice(WasmEdge_BatchContext *C, const WasmEdge_String *FuncNames,
                                             const uint32_t NumFuncs, const enum WasmEdge_ValType *const *ParamTypes,
                                             const uint32_t *ParamLens, const uint32_t *FuncOf,
                                             const uint64_t *Slots, const uint64_t Stride) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty())
    return R(C->fail(kRuntimeError, "a device buffer cannot serve a multi-device context: use BatchSetCalls"));
  if (!FuncOf || (NumFuncs && !FuncNames))
    return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: null FuncOf / FuncNames"));
  if ((ParamTypes == nullptr) != (ParamLens == nullptr))
    return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: ParamTypes and ParamLens go together"));
  DevScope dev(C);
  const wb::Program &P = C->prog;
  // each name's verdict, for the per-name table (sig_layout.h)
  std::vector<wb::CallName> names(NumFuncs);
  Staging s;
  uint64_t widest = 0;
  for (uint32_t j = 0; j < NumFuncs; j++) {
    const std::string name = str(FuncNames[j]);
    const int f = wb::find_export(P, name);
    names[j].status = kFuncNotFound;
    if (f < 0) continue;
    const wb::FuncInfo &F = P.funcs[f];
    const wb::FuncType &t = P.types[F.type];
    const wb::SigLayout L = wb::layout_of(t);
    if (L.param_xref || L.result_xref)
      return R(C->fail(kRuntimeError, "BatchSetCallsDevice: '" + name + "' takes or returns an externref, which is "
                                      "interned on the host: use BatchSetCalls"));
    widest = std::max<uint64_t>(widest, L.param_slots);
    // executor.cpp:88-100, on the type arrays: a device row carries no tags
    bool ok = true;
    if (ParamTypes) {
      ok = ParamLens[j] == t.params.size();
      if (ok && ParamLens[j] && !ParamTypes[j])
        return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: null ParamTypes row"));
      for (uint32_t k = 0; ok && k < ParamLens[j]; k++) ok = uint8_t(ParamTypes[j][k]) == t.params[k];
    }
    names[j].status = kFuncSigMismatch;
    if (!ok) continue;
    names[j] = wb::CallName{0, uint32_t(f), F.entry_pc, F.imported, &t};
    s.param_cells = std::max(s.param_cells, L.param_cells);
    s.result_cells = std::max(s.result_cells, L.result_cells);
    s.calls_res_slots = std::max(s.calls_res_slots, L.result_slots);
  }
  std::vector<uint32_t> tab = wb::calls_fn_table(names);
  if (widest && !Slots) return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: null Slots"));
  if (Stride < widest) return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: Stride is smaller than the widest row"));
  if ((uintptr_t(Slots) & 7u)) return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: Slots is not 8-byte aligned"));
  if ((uintptr_t(FuncOf) & 3u)) return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: FuncOf is not 4-byte aligned"));
  if (widest && Stride > (~0ull >> 4)) return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: Stride out of range"));
  if (!device_rows_ok(C, FuncOf, 4, 4, "BatchSetCallsDevice") ||
      !device_rows_ok(C, Slots, widest * 8, Stride * 8, "BatchSetCallsDevice"))
    return R(kRuntimeError);
  // the spare buffers the kernel writes; the result rows change size only on success
  if (!s.param_cells) s.param_cells = 1;
  const size_t rn = rows(C, s.result_cells);
  DevBuf<uint32_t> results;
  if (!sized(C->params_spare, rows(C, s.param_cells)) || !sized(C->calls_spare, size_t(C->n) * 2) ||
      !sized(C->call_fn_spare, C->n) || !sized(C->calls_sum, 1) ||
      ((C->results.n != rn || !C->results.ptr) && !results.alloc(rn))) {
    (void)hipGetLastError();
    return R(C->fail(kRuntimeError, "device allocation failed"));
  }
  if (!upload_map(C, C->calls_tab, C->calls_tab_h, tab)) return R(kRuntimeError);
  CallsPackParams p{};
  p.func_of = FuncOf;
  p.slots = Slots;
  p.table = C->calls_tab.ptr;
  p.calls = C->calls_spare.ptr;
  p.params = C->params_spare.ptr;
  p.call_fn = C->call_fn_spare.ptr;
  p.sum = C->calls_sum.ptr;
  p.stride = Stride;
  p.n = C->n;
  p.pc = s.param_cells;
  p.nfuncs = NumFuncs;
  if (!C->hip_ok(hipMemsetAsync(C->calls_sum.ptr, 0, sizeof(CallsSummary), C->stream), "call summary") ||
      !C->hip_ok(wb_launch_calls_pack(&p, C->stream), "calls pack") ||
      !C->hip_ok(hipMemcpyAsync(&C->calls_sum_h, C->calls_sum.ptr, sizeof(CallsSummary), hipMemcpyDeviceToHost,
                                C->stream), "call summary") ||
      !C->hip_ok(hipStreamSynchronize(C->stream), "calls pack"))
    return R(kRuntimeError);
  if (C->calls_sum_h.bad)
    return R(C->fail(kWrongVMWorkflow, "BatchSetCallsDevice: FuncOf[" + std::to_string(~C->calls_sum_h.bad) +
                                       "] names no function"));
  swap_bufs(C->params, C->params_spare);
  swap_bufs(C->calls, C->calls_spare);
  swap_bufs(C->call_fn, C->call_fn_spare);
  if (results.ptr) swap_bufs(C->results, results);
  // the vector's and the cells' order-independent sum: equal for equal device vectors, not
  // the value BatchSetCalls gives the same vector. call_func / call_status: fetched on first
  // need (calls_mirror)
  s.args_fp = args_fp_mix(~uint64_t(1), 0xC0C0C0C0u) + C->calls_sum_h.fp;
  s.calls_import = C->calls_sum_h.imported != 0;
  return commit_calls(C, s, false);
}

WasmEdge_Result WasmEdge_BatchCallsResultsDevice(WasmEdge_BatchContext *C, uint64_t *Slots, const uint32_t Width,
                                                 const uint64_t Stride, uint32_t *ReturnLens, uint8_t *PerInstance,
                                                 uint64_t *InstrCounts) {
  if (!C) return R(kWrongVMWorkflow);
  if (!C->shards.empty())
    return R(C->fail(kRuntimeError, "a device buffer cannot serve a multi-device context: use BatchResults"));
  const Staging &s = C->staged;
  if (!s.calls_on)
    return R(C->fail(kWrongVMWorkflow, "BatchCallsResultsDevice: no per-instance calls are staged: use BatchResultsDevice"));
  if (!C->ran) return R(C->fail(kWrongVMWorkflow, "BatchRun not called"));
  if (Slots && Stride < Width) return R(C->fail(kWrongVMWorkflow, "BatchCallsResultsDevice: Stride is smaller than Width"));
  if (Slots && Width < s.calls_res_slots)
    return R(C->fail(kWrongVMWorkflow, "BatchCallsResultsDevice: Width is smaller than the widest result row (" +
                                       std::to_string(s.calls_res_slots) + " slots)"));
  if ((uintptr_t(Slots) & 7u) || (uintptr_t(InstrCounts) & 7u) || (uintptr_t(ReturnLens) & 3u))
    return R(C->fail(kWrongVMWorkflow, "BatchCallsResultsDevice: a misaligned pointer"));
  if (Slots && Width && Stride > (~0ull >> 4))
    return R(C->fail(kWrongVMWorkflow, "BatchCallsResultsDevice: Stride out of range"));
  if (Slots && s.calls_xref)
    return R(C->fail(kRuntimeError, "BatchCallsResultsDevice: externref values are interned on the host: use BatchResults"));
  DevScope dev(C);
  const uint32_t width = Slots ? Width : 0;
  if (!device_rows_ok(C, Slots, uint64_t(width) * 8, Stride * 8, "BatchCallsResultsDevice") ||
      !device_rows_ok(C, ReturnLens, 4, 4, "BatchCallsResultsDevice") ||
      !device_rows_ok(C, PerInstance, 1, 1, "BatchCallsResultsDevice") ||
      !device_rows_ok(C, InstrCounts, 8, 8, "BatchCallsResultsDevice"))
    return R(kRuntimeError);
  // (every launch and host-import round of the run has ended: launch_once waits for its
  // kernel, a restore of a suspended invocation for its own)
  if (width || ReturnLens) {
    // each instance's function on the device: there already after SetCallsDevice, uploaded
    // after BatchSetCalls or a restore that rewrote call_func on the host
    if (!C->call_dev_ok) {
      if (!sized(C->call_fn, C->n)) {
        (void)hipGetLastError();
        return R(C->fail(kRuntimeError, "device allocation failed"));
      }
      if (!C->hip_ok(hipMemcpyAsync(C->call_fn.ptr, s.call_func.data(), size_t(C->n) * 4, hipMemcpyHostToDevice,
                                    C->stream), "call vector upload"))
        return R(kRuntimeError);
      C->call_dev_ok = true;
    }
    // the module's result table (sig_layout.h), built and uploaded once
    if (C->res_tab_h.empty()) {
      std::vector<const wb::FuncType *> types;
      for (const wb::FuncInfo &F : C->prog.funcs) types.push_back(&C->prog.types[F.type]);
      std::vector<uint32_t> tab = wb::calls_res_table(types);
      if (!upload_map(C, C->res_tab, C->res_tab_h, tab)) return R(kRuntimeError);
    }
    CallsUnpackParams p{};
    p.results = C->results.ptr;
    p.status = C->status.ptr;
    p.call_fn = C->call_fn.ptr;
    p.table = C->res_tab.ptr;
    p.slots = Slots;
    p.lens = ReturnLens;
    p.stride = Stride;
    p.n = C->n;
    p.cells = s.result_cells;
    p.width = width;
    if (!C->hip_ok(wb_launch_calls_unpack(&p, C->stream), "results unpack")) return R(kRuntimeError);
  }
  return finish_device_results(C, PerInstance, InstrCounts);
}

}  // extern "C"
