/*
 * wasmedge_batch.h -- C ABI of the MI355X batched WebAssembly interpreter.
 *
 * A batched entry placed BESIDE the reference's WasmEdge_VMExecute
 * (include/api/wasmedge/wasmedge.h:3301-3303, lib/api/wasmedge.cpp:2687-2698): one
 * validated module, N independent instances, one GPU lane each.  Conventions follow the
 * reference C API (include/api/wasmedge/wasmedge.h:39-60):
 *   - values are WasmEdge_Value {uint128_t Value; enum WasmEdge_ValType Type};
 *   - errors are returned by value as WasmEdge_Result{uint8_t Code} holding the
 *     reference ErrCode byte (include/common/enum.inc:573-749);
 *   - buffers are caller-owned; surplus returns are dropped, a ReturnLen shortfall is
 *     silent (lib/api/wasmedge.cpp:245-255 fillWasmEdge_ValueArr);
 *   - a NULL context gives WrongVMWorkflow (0x04) (lib/api/wasmedge.cpp:266-277);
 *   - contexts returned by *Create are owned by the caller and freed by *Delete.
 * Per-instance outcomes (traps) are reported per lane with the reference trap codes
 * (0x84..0x8E), never through the call-level result.
 *
 * Plain C types only; no torch/HIP types cross this boundary.
 */
#ifndef WASMEDGE_BATCH_H
#define WASMEDGE_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef WASMEDGE_C_API_H /* use the reference's definitions when its header is included */
typedef unsigned __int128 uint128_t;
enum WasmEdge_ValType {
  WasmEdge_ValType_I32 = 0x7FU,
  WasmEdge_ValType_I64 = 0x7EU,
  WasmEdge_ValType_F32 = 0x7DU,
  WasmEdge_ValType_F64 = 0x7CU,
  WasmEdge_ValType_V128 = 0x7BU,
  WasmEdge_ValType_FuncRef = 0x70U,
  WasmEdge_ValType_ExternRef = 0x6FU
};
typedef struct WasmEdge_Value {
  uint128_t Value;
  enum WasmEdge_ValType Type;
} WasmEdge_Value;
typedef struct WasmEdge_String {
  uint32_t Length;
  const char *Buf;
} WasmEdge_String;
typedef struct WasmEdge_Result {
  uint8_t Code;
} WasmEdge_Result;
#endif

#define WASMEDGE_BATCH_API __attribute__((visibility("default")))

/* Per-instance status byte (PerInstance[i]) beyond the reference trap codes. */
#define WASMEDGE_BATCH_OK 0x00u
#define WASMEDGE_BATCH_INTERRUPTED 0x07u      /* ErrCode::Interrupted: step/time limit */
#define WASMEDGE_BATCH_STACK_EXHAUSTED 0xB0u  /* device call stack full */
#define WASMEDGE_BATCH_HOST_CALL 0xB1u        /* reached a host import no host function is bound to */

typedef struct WasmEdge_BatchConfigure {
  /* Page limit per instance: RuntimeConfigure::MaxMemPage (include/common/configure.h:
   * 112-123; 0 = its default, 65536). memory.grow returns -1 past it, past the module's
   * declared maximum and past 65536 pages, or when the device has no memory left for the
   * new pages -- MemoryInstance::growPage (include/runtime/instance/memory.h:87-115) with
   * Allocator::resize failing (lib/system/allocator.cpp:101-129). Pages are committed on
   * demand, as the reference's mmap'd reservation is: see MemoryReservePages. A module
   * whose initial size exceeds a non-zero limit fails WasmEdge_BatchCreate with
   * MemoryOutOfBounds (0x88): the reference allocates no memory for it (memory.h:46-51). */
  uint32_t MaxMemoryPage;
  /* Device call-stack depth per instance in 32-bit cells. 0 (the default): the stack
   * starts at 4096 cells and grows on demand, as the reference's StackManager vectors do
   * (include/runtime/stackmgr.h:44-47) -- a call past it parks the instance, the stack
   * doubles between launches and the call runs again (counted once); only when the device
   * has no memory left for it does a call end the instance with 0xB0. Non-zero: a fixed
   * bound, 0xB0 past it. */
  uint32_t CallStackCells;
  /* Instruction budget per instance (0 = unlimited; counted in the reference's
   * Statistics units; checked every scheduler round, and a device-side core call never
   * runs a lane more than one compiled run past its remaining budget) and wall-clock limit per
   * launch in seconds (0 = 600); exceeding either marks the instance Interrupted (0x07),
   * mirroring the reference's cost limit / StopToken (statistics.h:69-91,
   * helper.cpp:24-27). */
  uint64_t MaxSteps;
  double TimeLimitSeconds;
  /* HIP device ordinal (-1 = the current device). */
  int32_t DeviceOrdinal;
  /* Gas limit per instance (StatisticsConfigure::setCostLimit, statistics.h:32,69-91;
   * 0 = no metering). Every wasm instruction adds its cost to the instance's running
   * total; the first one that would take the total past CostLimit fails with
   * CostLimitExceeded (0x03), counted but not executed (engine.cpp:1616-1630). The total
   * starts at instantiation, whose constant expressions and start function spend gas too,
   * and runs on across Execute/Run calls until BatchReset, like the reference VM's
   * Statistics::CostSum. Metered contexts run the compiled runs, which price themselves
   * exactly, and the per-lane step (no SIMT scheduling). */
  uint64_t CostLimit;
  /* Host threads serving lanes parked at host imports. 0 or 1: one thread, host
   * functions are called one at a time. More: waves are spread over that many threads
   * (a wave's lanes stay on one), so host functions must then be reentrant, as the
   * reference's are under concurrent VM::execute. */
  uint32_t HostThreads;
  /* Cost per instruction, indexed by the reference's OpCode (include/common/enum.inc:
   * one-byte opcodes, 0xFCxx, 0xFDxx): CostTableLen entries, the rest 0 -- the batched
   * WasmEdge_StatisticsSetCostTable (lib/api/wasmedge.cpp:878-882, statistics.h:59-66).
   * NULL with length 0: the default table, every instruction costs 1. Copied at
   * BatchCreate. */
  const uint64_t *CostTable;
  uint32_t CostTableLen;
  /* Bytes per granule in which the device interleaves the linear memories of a wave's 64
   * instances (4, 8, ..., 128; 0 = chosen: 4 when the module's load/store addresses are the
   * same in every instance; when an address may depend on per-instance data, a layout trial
   * decides from measured throughput -- the first Run is an unmeasured warm-up at 128, the
   * second is measured at 128, the next Reset re-lays memory in 4-byte words and the Run
   * after it is measured again; 4 stays if at least 10% faster per wasm instruction on the
   * same function, else the following Reset goes back to 128 (WB_GRANULE_TRIAL=0: 128, no
   * trial). The shards of a multi-device batch take the first shard's verdict.) Layout
   * only: results never depend on it. WasmEdge_BatchGetMemoryGranule reports the layout in
   * use. */
  uint32_t MemoryGranule;
  /* The TailCall proposal (return_call, return_call_indirect; WasmEdge_ConfigureAddProposal
   * (Conf, WasmEdge_Proposal_TailCall), include/common/configure.h:176-182 leaves it off):
   * 0 = off, the opcodes fail BatchCreate with IllegalOpCode (0x37) as in the reference's
   * loader. On: a tail call reuses the caller's frame, so tail recursion never exhausts the
   * device call stack; a host import in tail position runs on the yield path and its results
   * return from the caller (DESIGN.md "Tail calls"). */
  uint32_t TailCall;
  /* Layout of linear memory on the device (results never depend on it). The first
   * MemoryReservePages pages of every instance are allocated up front in the lane-
   * interleaved layout every execution path addresses directly; pages an instance grows
   * past them are committed on demand in 4 MiB rows (the page for all 64 instances of a
   * wave) and reached through a page table by the per-lane step, more slowly. 0 = the
   * module's initial size, raised toward the page limit while the whole batch's
   * reservation stays within min(16 GiB, a quarter of the device's free memory); modules
   * without memory.grow reserve their initial size. Clamped to [initial size, limit]. After
   * a run whose instances grew past it, the next BatchReset re-lays memory with the largest
   * size they reached in the reserved layout (WasmEdge_BatchGetReservedPages), so later runs
   * address every page directly. */
  uint32_t MemoryReservePages;
  /* Cap on the device memory committed for grown pages (bytes; 0 = until hipMalloc fails).
   * A grow that would need more returns -1. */
  uint64_t MemoryPoolBytes;
  /* Devices the batch spreads over from this one process (SURVEY.md 8(b) NumDevices, 8(e)).
   * DeviceCount 0 or 1: one device, DeviceOrdinal. More: Devices[0..DeviceCount) are HIP
   * ordinals -- a device may repeat (several shards on one device) -- and instance ids go to
   * them by Partition: WASMEDGE_BATCH_PARTITION_BLOCKS, contiguous blocks of whole waves, or
   * WASMEDGE_BATCH_PARTITION_INTERLEAVE, id mod DeviceCount (evens out work that varies
   * with the id). Every call then drives every shard -- one host thread and one stream per
   * shard, no collective -- and gathers per-instance outputs into the caller's
   * [NumInstances] arrays in instance order (WasmEdge_BatchPlacement gives the map).
   * Results never depend on it; like the reference's concurrent VM::execute
   * (include/vm/vm.h:137-141), host functions are called from one shard at a time unless
   * HostThreads > 1. */
  const int32_t *Devices;
  uint32_t DeviceCount;
  uint32_t Partition;
  /* The MultiMemories proposal (WasmEdge_ConfigureAddProposal(Conf,
   * WasmEdge_Proposal_MultiMemories), include/common/enum.inc:555; off by default,
   * configure.h:176-182): 0 = off, a second memory fails BatchCreate with MultiMemories
   * (0x51, validator.cpp:107-113). On: several memories (defined or imported) and memory
   * indices in loads, stores, memory.size/grow/fill/copy/init and data segments, read as
   * the reference reads them (a memarg's index after its offset, instruction.cpp:144-156).
   * Memory 0 keeps every execution path; instructions on the other memories run in the
   * per-lane step, on memories reserved whole per instance (their initial size, or up to
   * their limit as far as min(4 GiB, free/8) per batch goes when the module grows them; a
   * grow past that returns -1). WasmEdge_BatchGetMemory / the memory hash cover memory 0. */
  uint32_t MultiMemories;
  /* Pages reserved per instance for each memory past the first that the module grows
   * (0 = chosen as above: the page limit as far as min(4 GiB, free/8) for the whole batch
   * goes -- with tens of thousands of instances that can be few or none, and then
   * memory.grow on it returns -1 where the reference's would succeed). Clamped to [initial
   * size, limit]; BatchCreate fails with RuntimeError when the batch does not fit.
   * WasmEdge_BatchGetExtraMemoryPages reports the reservation in use. */
  uint32_t ExtraMemoryReservePages;
  /* Cap on the device memory the call stack may grow to when CallStackCells is 0 (bytes;
   * 0 = an eighth of the device's memory). Past it a call ends the instance with 0xB0.
   * Each BatchReset returns the stack to its first depth. */
  uint64_t CallStackMaxBytes;
  /* Resumable runs (WasmEdge_BatchResume below): 0 = off, Interrupted (0x07) is final and
   * BatchResume fails with WrongVMWorkflow (0x04). Non-zero: an instance that ends a
   * BatchRun or BatchResume with 0x07 is suspended on the device, and the frame-save area
   * is allocated for every module, not only those with imports or growth. */
  uint32_t Resumable;
} WasmEdge_BatchConfigure;

#define WASMEDGE_BATCH_PARTITION_BLOCKS 0u
#define WASMEDGE_BATCH_PARTITION_INTERLEAVE 1u

/* Where instance Inst of a NumInstances-instance batch over DeviceCount devices runs: the
 * index into Devices (*Shard) and its lane on that device (*Local). No device is touched.
 * WrongVMWorkflow (0x04) for Inst >= NumInstances, DeviceCount 0 or an unknown Partition. */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchPlacement(uint32_t NumInstances, uint32_t DeviceCount,
                                                          uint32_t Partition, uint32_t Inst,
                                                          uint32_t *Shard, uint32_t *Local);

#ifdef WASMEDGE_C_API_H
/* The reference's configuration object as a batch configuration (header-inline: needs the
 * reference's wasmedge.h included first). It carries over what the reference's
 * WasmEdge_ConfigureContext decides for the interpreter path: the page limit
 * (WasmEdge_ConfigureGetMaxMemoryPage, wasmedge.h:560; RuntimeConfigure::MaxMemPage,
 * configure.h:112-123) and the TailCall and MultiMemories proposals
 * (WasmEdge_ConfigureHasProposal, wasmedge.h:495; off by default, configure.h:176-182).
 * The proposals on by default (SIMD, bulk memory, reference types, multi-value, sign
 * extension, saturating conversions, mutable globals) are always on in the batched path.
 * Statistics: instruction counts are always reported;
 * cost metering is set through CostLimit / CostTable (the reference keeps those on its
 * StatisticsContext). Fields this does not set keep the caller's values; a NULL Conf
 * leaves the reference defaults (MaxMemoryPage 0 = 65536, TailCall and MultiMemories off). */
static inline void WasmEdge_BatchConfigureFromContext(const WasmEdge_ConfigureContext *Conf,
                                                      WasmEdge_BatchConfigure *Out) {
  if (!Out) return;
  if (!Conf) {
    Out->MaxMemoryPage = 0;
    Out->TailCall = 0;
    Out->MultiMemories = 0;
    return;
  }
  Out->MaxMemoryPage = WasmEdge_ConfigureGetMaxMemoryPage(Conf);
  Out->TailCall = WasmEdge_ConfigureHasProposal(Conf, WasmEdge_Proposal_TailCall) ? 1u : 0u;
  Out->MultiMemories = WasmEdge_ConfigureHasProposal(Conf, WasmEdge_Proposal_MultiMemories) ? 1u : 0u;
}
#endif

typedef struct WasmEdge_BatchContext WasmEdge_BatchContext;

/* Load + validate + lower `WasmBuf`, allocate device state for NumInstances instances
 * and instantiate them (BatchReset). Replaces VM::loadWasm/validate/instantiate
 * (lib/vm/vm.cpp) for the batch. Returns NULL on failure with the ErrCode in *Res (may
 * be NULL). */
WASMEDGE_BATCH_API WasmEdge_BatchContext *
WasmEdge_BatchCreate(const WasmEdge_BatchConfigure *Conf, const uint8_t *WasmBuf,
                     uint32_t WasmLen, uint32_t NumInstances, WasmEdge_Result *Res);

/* A table, memory or global the embedder provides for the module's imports of that
 * kind -- the batched form of creating it (WasmEdge_TableInstanceCreate /
 * MemoryInstanceCreate / GlobalInstanceCreate, wasmedge.h) and adding it to an import
 * object (WasmEdge_ImportObjectAddTable/AddMemory/AddGlobal). Every instance gets a copy
 * of its own, as each reference VM has its own import object: a memory of Min zeroed
 * pages, a table of Min null references, a global holding Value. Matching follows
 * lib/executor/instantiate/import.cpp: an import with no provider fails with UnknownImport
 * (0x62); a provider of another reference / value type or mutability, or whose limits do
 * not fit the import's (Min >= the import's min; a Max when the import has one, no larger),
 * fails with IncompatibleImportType (0x61). Function imports bind later, through
 * WasmEdge_BatchAddHostFunction / WasmEdge_BatchInitWASI. */
#define WASMEDGE_BATCH_IMPORT_TABLE 1u
#define WASMEDGE_BATCH_IMPORT_MEMORY 2u
#define WASMEDGE_BATCH_IMPORT_GLOBAL 3u
typedef struct WasmEdge_BatchImport {
  WasmEdge_String ModuleName;
  WasmEdge_String ExternalName;
  uint32_t Kind;                /* WASMEDGE_BATCH_IMPORT_* (the reference ExternalType) */
  uint32_t Min, Max;            /* table / memory limits */
  uint32_t HasMax;
  enum WasmEdge_ValType Type;   /* table: FuncRef / ExternRef; global: its value type */
  uint32_t Mutable;             /* global: 1 = var */
  WasmEdge_Value Value;         /* global: its initial value (a funcref is a function
                                   index of the module, an externref any 64-bit value,
                                   null 0xFFFFFFFF) */
} WasmEdge_BatchImport;

/* WasmEdge_BatchCreate with the module's table / memory / global imports provided. */
WASMEDGE_BATCH_API WasmEdge_BatchContext *
WasmEdge_BatchCreateWithImports(const WasmEdge_BatchConfigure *Conf, const uint8_t *WasmBuf,
                                uint32_t WasmLen, uint32_t NumInstances,
                                const WasmEdge_BatchImport *Imports, uint32_t ImportLen,
                                WasmEdge_Result *Res);

/* Run `FuncName` on every instance (one instance per lane). Instance state -- linear
 * memory and its size, globals, dropped data segments -- persists from one Execute/Run
 * to the next until BatchReset, as an instantiated module does in the reference VM.
 * Params: [NumInstances][ParamLen] row-major; Returns: [NumInstances][ReturnLen].
 * PerInstance[i]: 0 ok, else trap/status code. InstrCounts[i]: the reference's
 * instruction count (include/common/statistics.h:44). Either may be NULL.
 * Mirrors WasmEdge_VMExecute (wasmedge.h:3301) per instance. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchExecute(WasmEdge_BatchContext *Cxt, const WasmEdge_String FuncName,
                      const WasmEdge_Value *Params, const uint32_t ParamLen,
                      WasmEdge_Value *Returns, const uint32_t ReturnLen,
                      uint8_t *PerInstance, uint64_t *InstrCounts);

/* SURVEY.md §8(b)'s form of the same call: the per-instance outcome as a WasmEdge_Result
 * each (Code = the status byte above). WasmEdge_Result is one byte (wasmedge.h:55-60), so
 * an array of them is the status array itself. */
typedef char WasmEdge_BatchResultIsOneByte[sizeof(WasmEdge_Result) == 1 ? 1 : -1];
static inline WasmEdge_Result
WasmEdge_BatchExecuteResults(WasmEdge_BatchContext *Cxt, const WasmEdge_String FuncName,
                             const WasmEdge_Value *Params, const uint32_t ParamLen,
                             WasmEdge_Value *Returns, const uint32_t ReturnLen,
                             WasmEdge_Result *PerInstance, uint64_t *InstrCounts) {
  return WasmEdge_BatchExecute(Cxt, FuncName, Params, ParamLen, Returns, ReturnLen,
                               (uint8_t *)PerInstance, InstrCounts);
}

/* Ask a running BatchExecute/BatchRun on this context to stop (any thread): every
 * instance still running ends with Interrupted (0x07) at the next scheduler round (the
 * flag is read every round; a core call runs at most 2^20 instructions), like the
 * reference's StopToken / async cancel (helper.cpp:24-27, include/common/async.h:73-77).
 * The request is cleared when the next Run starts. */
WASMEDGE_BATCH_API void WasmEdge_BatchInterrupt(WasmEdge_BatchContext *Cxt);

/* Staged form of BatchExecute, for callers that keep inputs resident on the device
 * and time the interpreter alone (bench.py):
 *   SetArgs  -> resolve FuncName, check types (FuncSigMismatch), upload params
 *   Reset    -> fresh instances: memory image, globals, then the start function
 *               (lib/executor/instantiate/module.cpp:16-172); a lane whose start
 *               function traps reports that trap from every later Run.
 *               *KernelSeconds = the reset kernels' time; NULL: Reset does not wait
 *               for them (without a start function), the next Run orders after them
 *   Run      -> launch the interpreter; *KernelSeconds = HIP-event time on the
 *               library's stream (may be NULL)
 *   Results  -> copy returns / statuses / counts back. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSetArgs(WasmEdge_BatchContext *Cxt, const WasmEdge_String FuncName,
                      const WasmEdge_Value *Params, const uint32_t ParamLen);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchReset(WasmEdge_BatchContext *Cxt,
                                                       double *KernelSeconds);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchRun(WasmEdge_BatchContext *Cxt,
                                                     double *KernelSeconds);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchResults(WasmEdge_BatchContext *Cxt, WasmEdge_Value *Returns,
                      const uint32_t ReturnLen, uint8_t *PerInstance, uint64_t *InstrCounts);

/* ---- device-resident arguments and results ----------------------------------------------
 * SetArgs and Results for a caller whose inputs are produced, and whose outputs are consumed,
 * on the device (a torch pipeline, a search loop feeding BatchSnapshotRestore): the values
 * never cross the host. Between them BatchReset, BatchRun and BatchResume work as ever, and
 * either call may be mixed with its host variant.
 *
 * The device value format is the SLOT form: one value is one 64-bit little-endian slot, a
 * v128 two slots, low half first. A slot holds the low 64 bits of the WasmEdge_Value.Value
 * the host variants take or return: i32, f32 and funcref in its low 32 bits (on input the
 * upper 32 bits are ignored, as BatchSetArgs ignores them; on output they are zero), f32 and
 * f64 as their bit patterns, a null funcref as 0xFFFFFFFF. A row is the function's values
 * back to back; Slots is [NumInstances][Stride] uint64 (for torch: an int64 tensor), 8-byte
 * aligned, Stride counted in slots and at least the slots of a row.
 *
 * BatchSetArgsDevice has the semantics of BatchSetArgs: FuncNotFound (0x05) for an unknown
 * export; FuncSigMismatch (0x83) when ParamLen or ParamTypes -- a HOST array, checked in
 * place of the tags a device row does not carry -- differ from the function's signature; it
 * returns to one function for every instance, ends a suspended invocation, and keeps the
 * device buffers of the arguments and results when their sizes do not change. A function
 * without parameters is legal with NULL Slots.
 *
 * BatchResultsDevice works wherever BatchResults works: after BatchRun or BatchResume, at
 * once after the restore of a suspended snapshot, after BatchSetArgs as well as after
 * BatchSetArgsDevice. Row i receives the first min(ReturnLen, result count) values of
 * instance i; the slots of a row past them and the padding up to Stride are left untouched.
 * An instance whose status is not 0 (a trap, 0x07 -- suspended or final --, CostLimitExceeded)
 * gets zeroes in those slots, as BatchResults zeroes its values. Slots may be NULL (no
 * values). PerInstance (device, [NumInstances] bytes) and InstrCounts (device,
 * [NumInstances] uint64), each may be NULL, are plain device-to-device copies of what
 * BatchResults returns in their host namesakes.
 *
 * WrongVMWorkflow (0x04), for both calls: a NULL context, a Stride smaller than the row
 * needs, a misaligned pointer; for SetArgsDevice, NULL Slots with a non-empty row; for
 * ResultsDevice, no completed run, and per-instance calls (their rows differ in signature:
 * BatchCallsResultsDevice below reads them). RuntimeError (0x02): a function with an externref
 * parameter or result (wide externrefs are interned on the host: use the host variants); a
 * multi-device context (one device buffer cannot serve several devices); a buffer this HIP
 * runtime knows not to be on the context's device or not to hold NumInstances rows. Every
 * failure leaves the staging, the results and the caller's buffers as they were and sets the
 * WasmEdge_BatchGetLastError message.
 *
 * Ordering, as for the *MemoriesDevice calls: the CALLER makes sure that whatever produced
 * the buffer has finished before the call (synchronise the stream that wrote it); the library
 * synchronises its own stream before it returns, so the rows are complete, and after every
 * host-import round of the run, when ResultsDevice returns.
 *
 * The arguments' fingerprint -- it decides whether a learnt longest-first wave order is
 * reused, and whether BatchRun after the restore of a suspended snapshot asks for a new
 * staging -- is computed on the device from the staged cells and the function: equal for
 * equal device arguments, different for different ones. It is NOT the value BatchSetArgs
 * gives the same arguments: staging the same values once by each path counts as a change
 * (the wave order is learnt again; a restored invocation wants its arguments staged by the
 * path that staged them before the capture). Results never depend on it. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSetArgsDevice(WasmEdge_BatchContext *Cxt, const WasmEdge_String FuncName,
                            const enum WasmEdge_ValType *ParamTypes /* host */,
                            const uint32_t ParamLen, const uint64_t *Slots /* device */,
                            const uint64_t Stride /* slots per row */);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchResultsDevice(WasmEdge_BatchContext *Cxt, uint64_t *Slots /* device, may be NULL */,
                            const uint32_t ReturnLen, const uint64_t Stride,
                            uint8_t *PerInstance /* device [N], may be NULL */,
                            uint64_t *InstrCounts /* device [N], may be NULL */);

/* ---- device-resident per-instance calls -------------------------------------------------
 * BatchSetCalls and its results (below, "per-instance calls") for a caller whose call vector
 * and arguments are produced on the device -- "reset the finished environments, step the
 * others" without a trip through the host. The names, and optionally their signatures, are
 * host arrays of NumFuncs entries; FuncOf and the rows are device buffers.
 *
 * BatchSetCallsDevice has the semantics of BatchSetCalls. FuncOf is a DEVICE array
 * [NumInstances] of indices into FuncNames or WASMEDGE_BATCH_NO_CALL. Slots is
 * [NumInstances][Stride] in the slot form above: row i holds the parameters of
 * FuncNames[FuncOf[i]] back to back from slot 0 (one slot per value, two for a v128, the upper
 * half of an i32 / f32 / funcref slot ignored); what a row holds past them is not read. Per
 * instance: NO_CALL gives status 0 and the instance does not run; a name that is no exported
 * function gives FuncNotFound (0x05); with ParamTypes given (a host array of NumFuncs host
 * arrays, with ParamLens their lengths; both NULL: the module's signatures are taken as they
 * are), a ParamLens[j] / ParamTypes[j] that differs from function j's signature gives every
 * instance naming j FuncSigMismatch (0x83). None of the three runs, and its state stays
 * untouched. A named export that is a host import fails BatchRun (RuntimeError) only when some
 * instance calls it, as after BatchSetCalls.
 *
 * WrongVMWorkflow (0x04): a NULL context; NULL FuncOf, or NULL FuncNames with NumFuncs != 0;
 * exactly one of ParamTypes / ParamLens NULL; a Stride smaller than the widest parameter row
 * among the names that resolve; NULL Slots while a resolved function has parameters; a
 * misaligned pointer (8 bytes for Slots, 4 for FuncOf); some FuncOf[i] that is neither NO_CALL
 * nor < NumFuncs (the message names the lowest such i). RuntimeError (0x02): a named function
 * with an externref parameter or result, called or not; a multi-device context; a buffer this
 * HIP runtime knows not to be on the context's device or to be too small. Every failure leaves
 * the previous staging (still runnable), the results and the caller's buffers as they were and
 * sets the WasmEdge_BatchGetLastError message. A successful call ends a suspended invocation
 * and keeps the device buffers when their sizes do not change.
 *
 * BatchCallsResultsDevice works wherever BatchResults works after a per-instance staging:
 * after BatchRun / BatchResume, at once after the restore of a suspended snapshot that holds a
 * call vector, after BatchSetCalls as well as after BatchSetCallsDevice. Row i of Slots gets
 * exactly Width slots: its function's result slots first, then zeroes; an instance whose
 * status is not 0, or that sat the run out, gets Width zeroes; the padding from Width to
 * Stride is untouched. ReturnLens[i] (device, uint32) is what BatchGetReturnLens gives;
 * PerInstance and InstrCounts are device-to-device copies as for BatchResultsDevice. Each of
 * the four may be NULL (with NULL Slots, Width and Stride are not looked at).
 * WrongVMWorkflow (0x04), nothing written: a NULL context; no per-instance staging (a uniform
 * one: use BatchResultsDevice); no completed run; Stride < Width; a Width smaller than the
 * widest result row among the staging's functions; a misaligned pointer. RuntimeError (0x02):
 * a multi-device context; a wrong-device or short buffer; a function with an externref result
 * (possible only after the host BatchSetCalls).
 *
 * Ordering and the fingerprint: as for the calls above. The fingerprint covers FuncOf's
 * outcome per instance and every staged cell; it is not the value BatchSetCalls gives the same
 * vector. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSetCallsDevice(WasmEdge_BatchContext *Cxt, const WasmEdge_String *FuncNames,
                             const uint32_t NumFuncs /* host */,
                             const enum WasmEdge_ValType *const *ParamTypes /* host [NumFuncs], may be NULL */,
                             const uint32_t *ParamLens /* host [NumFuncs], NULL iff ParamTypes is */,
                             const uint32_t *FuncOf /* DEVICE [NumInstances] */,
                             const uint64_t *Slots /* DEVICE [NumInstances][Stride] */,
                             const uint64_t Stride);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchCallsResultsDevice(WasmEdge_BatchContext *Cxt, uint64_t *Slots /* device, may be NULL */,
                                 const uint32_t Width, const uint64_t Stride,
                                 uint32_t *ReturnLens /* device [N], may be NULL */,
                                 uint8_t *PerInstance /* device [N], may be NULL */,
                                 uint64_t *InstrCounts /* device [N], may be NULL */);

/* ---- resumable runs ---------------------------------------------------------------------
 * With WasmEdge_BatchConfigure::Resumable set, an instance that ends a BatchRun or a
 * BatchResume with Interrupted (0x07) -- MaxSteps / StepLimit reached, TimeLimitSeconds
 * passed, WasmEdge_BatchInterrupt -- is SUSPENDED, not lost: it keeps 0x07 in PerInstance
 * and its count so far in InstrCounts, its returns read zero, and its frame, call stack, pc,
 * gas total and instance state stay on the device. The reference has no counterpart (its
 * Interrupted is final), hence the switch.
 *
 * BatchResume continues every suspended instance from where it stopped, in one launch
 * followed by the usual host-import rounds. Every other instance -- finished, trapped,
 * CostLimitExceeded (0x03), or sat out with NO_CALL / FuncNotFound / FuncSigMismatch -- is
 * untouched: status, count, returns, memory and gas stay as they were. StepLimit is the new
 * CUMULATIVE per-instance instruction limit of the invocation, in the units of InstrCounts
 * (which run on across resumes); 0 = none. A caller slices with k * slice. An instance whose
 * count already reaches StepLimit is suspended again as it is; one below it retires at least
 * one instruction. The wall-clock limit starts anew with each call, and a pending interrupt
 * request is cleared when the call starts, as in BatchRun. With nothing suspended the call
 * succeeds and launches nothing (*KernelSeconds = 0). BatchResults afterwards works as after
 * BatchRun; per-instance calls keep their ReturnLens.
 *
 * BatchGetSuspendedCount: the suspended instances after the last Run / Resume (a counter
 * the kernels keep; no status copy), 0 for NULL; a multi-device context sums its shards.
 *
 * BatchReset, BatchSetArgs, BatchSetCalls and BatchSnapshotRestore end a suspended
 * invocation: BatchResume then fails with WrongVMWorkflow (0x04), as it does on a context
 * that is not Resumable, before any BatchRun, and for NULL. BatchRun ends it too and begins a
 * new one: what it left suspended is dropped, and a BatchResume after it continues the
 * instances the new run suspended. BatchSnapshotCreate stays legal
 * (it captures no frames: restoring such a snapshot equals restoring one taken between
 * runs, and ends the invocation). BatchSnapshotCreateSuspended (below) captures the
 * suspended invocation as well; restoring such a snapshot reinstates it, whatever ended it
 * since, and BatchResume continues it. Between slices a caller may read (BatchResults, GetMemory, ReadMemories(Device),
 * MemoryHash, GlobalGetValue, TableGet*, GetTotalCosts) and write (SetMemory,
 * WriteMemories(Device), GlobalSetValue, TableSetData); a suspended instance sees the
 * writes when it continues, as if a host function had made them. Not resumable: a start
 * function interrupted during BatchReset (0x07 stays the instantiation status) and
 * CostLimitExceeded. */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchResume(WasmEdge_BatchContext *Cxt, uint64_t StepLimit,
                                                        double *KernelSeconds);
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetSuspendedCount(const WasmEdge_BatchContext *Cxt);

/* ---- per-instance calls ---------------------------------------------------------------
 * Each instance runs its own export: N independent WasmEdge_VMExecute calls
 * (wasmedge.h:3301) in one launch. FuncOf[i] indexes FuncNames, or is
 * WASMEDGE_BATCH_NO_CALL. Params is [NumInstances][ParamStride] row-major; instance i
 * passes the first ParamLens[i] values of its row (ParamLens NULL: ParamStride each).
 *   - a name that is not an exported function: FuncNotFound (0x05) in PerInstance[i]
 *     (lib/vm/vm.cpp:287-308);
 *   - a ParamLens[i] or value types that do not match the function: FuncSigMismatch (0x83)
 *     in PerInstance[i] (lib/executor/executor.cpp:88-100);
 *   - NO_CALL: status 0.
 * None of these three runs: instruction count 0, returns zeroed, its memory, globals,
 * tables and gas total untouched; the other instances run normally. The call itself fails
 * only on setup errors: a NULL context or a FuncOf[i] that is neither NO_CALL nor
 * < NumFuncs (WrongVMWorkflow 0x04, the previous staging intact), an externref that cannot
 * be interned, and -- at BatchRun -- a called export that is a host import.
 * After SetCalls, BatchRun and BatchResults work as after SetArgs: Results' ReturnLen is the
 * row stride, row i holds its function's results (their count: BatchGetReturnLens) with its
 * result types, then zeroed values. A later BatchSetArgs returns to one function for all. */
#define WASMEDGE_BATCH_NO_CALL 0xFFFFFFFFu
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSetCalls(WasmEdge_BatchContext *Cxt, const WasmEdge_String *FuncNames,
                       const uint32_t NumFuncs, const uint32_t *FuncOf,
                       const WasmEdge_Value *Params, const uint32_t ParamStride,
                       const uint32_t *ParamLens);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchExecuteCalls(WasmEdge_BatchContext *Cxt, const WasmEdge_String *FuncNames,
                           const uint32_t NumFuncs, const uint32_t *FuncOf,
                           const WasmEdge_Value *Params, const uint32_t ParamStride,
                           const uint32_t *ParamLens, WasmEdge_Value *Returns,
                           const uint32_t ReturnStride, uint32_t *ReturnLens /* may be NULL */,
                           uint8_t *PerInstance, uint64_t *InstrCounts);
/* ReturnLens[i]: the result count of instance i's function (0 for one that did not run). */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchGetReturnLens(WasmEdge_BatchContext *Cxt,
                                                               uint32_t *ReturnLens);

/* ---- host functions (the yield path) --------------------------------
 * A lane that calls an imported function parks on the device; BatchRun / BatchReset then
 * call the host function registered for that import on the CPU, once per parked lane,
 * write its results back and resume the lanes, until none is parked -- the batched form
 * of the reference's host-function call (lib/executor/helper.cpp:35-97,
 * include/runtime/hostfunc.h:25-40). The signature mirrors WasmEdge_HostFunc_t
 * (include/api/wasmedge/wasmedge.h:2269-2271); MemCxt is the calling instance's memory.
 * A non-zero Result ends that instance with the code in PerInstance (Terminated 0x01,
 * as from proc_exit, ends it "successfully" with zeroed returns; engine.cpp:62-64). An
 * import without a registered function ends the instance with 0xB1. */
typedef struct WasmEdge_BatchMemoryContext WasmEdge_BatchMemoryContext;
typedef WasmEdge_Result (*WasmEdge_BatchHostFunc_t)(void *Data,
                                                    WasmEdge_BatchMemoryContext *MemCxt,
                                                    const WasmEdge_Value *Params,
                                                    WasmEdge_Value *Returns);
/* Bind `Func` to every import named ModuleName.FuncName (WasmEdge_ImportObjectAddFunction,
 * wasmedge.h:2814). Register before the first Run (and before Reset when the start
 * function calls imports). */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchAddHostFunction(WasmEdge_BatchContext *Cxt, const WasmEdge_String ModuleName,
                              const WasmEdge_String FuncName, WasmEdge_BatchHostFunc_t Func,
                              void *Data);
/* The same with the host function's gas cost: the Cost of WasmEdge_FunctionInstanceCreate
 * (Type, Func, Data, Cost) (include/api/wasmedge/wasmedge.h:2324; HostFunctionBase::Cost,
 * include/runtime/hostfunc.h:28-46). In a metered context (CostLimit) every call adds Cost
 * to the instance's gas total before the function runs; a call that would take the total
 * past CostLimit ends the instance with CostLimitExceeded (0x03) instead -- the call
 * instruction counted, the host function not run, the total unchanged -- as
 * Stat->addCost(HostFunc.getCost()) does (lib/executor/helper.cpp:59-64). The built-in WASI
 * functions cost 0, as the reference's do (include/host/wasi/wasibase.h:15). */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchAddHostFunctionWithCost(WasmEdge_BatchContext *Cxt, const WasmEdge_String ModuleName,
                                      const WasmEdge_String FuncName, WasmEdge_BatchHostFunc_t Func,
                                      void *Data, uint64_t Cost);
/* Inside a host function: the calling instance and its memory
 * (WasmEdge_MemoryInstanceGetData / SetData, wasmedge.h:2552-2569). */
WASMEDGE_BATCH_API uint32_t
WasmEdge_BatchMemoryGetInstance(const WasmEdge_BatchMemoryContext *MemCxt);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchMemoryGetData(const WasmEdge_BatchMemoryContext *MemCxt, uint8_t *Data,
                            const uint32_t Offset, const uint32_t Length);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchMemorySetData(WasmEdge_BatchMemoryContext *MemCxt, const uint8_t *Data,
                            const uint32_t Offset, const uint32_t Length);

/* ---- built-in WASI subset (wasi_snapshot_preview1) on the yield path -------------------
 * Binds the module's imports args_get, args_sizes_get, environ_get, environ_sizes_get,
 * fd_write, proc_exit and sched_yield (those with the WASI signature) to host functions
 * inside the library, as WasmEdge_ImportObjectCreateWASI / InitWASI would
 * (include/api/wasmedge/wasmedge.h:2719-2754, lib/host/wasi/wasifunc.cpp), plus
 * fd_prestat_get and fd_prestat_dir_name. Args/Envs are shared by every instance unless an
 * instance has its own args (WasmEdge_BatchWASISetInstanceArgs). fd_write to fd 1 / 2 is
 * captured per instance (fd 0 gives NOTCAPABLE, other fds BADF); proc_exit records the exit code
 * and ends the instance with Terminated (0x01). Calling it again re-initialises the
 * environment and clears the captured output and exit codes. Other WASI imports stay
 * unbound (0xB1 when reached) unless registered with WasmEdge_BatchAddHostFunction. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchInitWASI(WasmEdge_BatchContext *Cxt, const char *const *Args, const uint32_t ArgLen,
                       const char *const *Envs, const uint32_t EnvLen);
/* The same with preopened directories, as WasmEdge_ImportObjectInitWASI's Preopens
 * (wasmedge.h:2739-2742): "guest:host" or one path for both; they become fds 3, 4, ... in
 * the order given (environ.cpp:54-93), named by VINode::canonicalGuest, with the
 * reference's rights, and behave as a read-only mount (N instances share the host
 * directory): path_open, fd_read, fd_seek, fd_tell, fd_close, fd_fdstat_get,
 * fd_filestat_get, path_filestat_get, fd_prestat_get / _dir_name work on them, an open that
 * would create, truncate or write fails with ROFS. A file is read whole when an instance
 * first opens it. Also bound: clock_time_get, clock_res_get, random_get,
 * fd_fdstat_set_flags (wasmedge_amd/csrc/wasi_impl.h lists each with its reference
 * lines). */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchInitWASIWithPreopens(WasmEdge_BatchContext *Cxt, const char *const *Args,
                                   const uint32_t ArgLen, const char *const *Envs,
                                   const uint32_t EnvLen, const char *const *Preopens,
                                   const uint32_t PreopenLen);
/* Instance Inst's own command line (args_get / args_sizes_get), in place of the shared Args:
 * the reference builds one Environ per VM (environ.cpp:95-98), so N instances with their
 * own arguments are N VMs with their own WASI modules. Call after WasmEdge_BatchInitWASI
 * (which clears every instance's own args). */
/* Reproducible WASI: instance i's new fd numbers and random_get bytes come from a
 * generator seeded by (Seed, i) -- the reference draws both from std::random_device
 * (environ.h:834-850, 1096-1108), and so does this library by default -- and every clock
 * reads ClockNs, advancing 1 us per call of the instance (clock_res_get: 1 ns). Call after
 * the InitWASI call it applies to; it also resets the instances' fd tables. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchWASISetDeterministic(WasmEdge_BatchContext *Cxt, uint64_t Seed, uint64_t ClockNs);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchWASISetInstanceArgs(WasmEdge_BatchContext *Cxt, uint32_t Inst,
                                  const char *const *Args, const uint32_t ArgLen);
/* proc_exit code of instance Inst (0 if it never called it; WasmEdge_ImportObjectWASIGetExitCode,
 * wasmedge.h:2754). */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchWASIGetExitCode(const WasmEdge_BatchContext *Cxt,
                                                          uint32_t Inst);
/* Bytes instance Inst wrote to fd 1 (stdout) or 2 (stderr); copies at most Len of them into
 * Buf (may be NULL) and returns the total size. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchWASIGetOutput(const WasmEdge_BatchContext *Cxt,
                                                        uint32_t Inst, uint32_t Fd, uint8_t *Buf,
                                                        uint32_t Len);

/* Each instance's gas total (WasmEdge_StatisticsGetTotalCost, wasmedge.h): Costs[N];
 * all 0 when the context does not meter. */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchGetTotalCosts(WasmEdge_BatchContext *Cxt,
                                                               uint64_t *Costs);

/* Straight-line runs of the module that the context compiled to machine code for the
 * V-frame threaded core (DESIGN.md "Compiled runs"; 0 when it runs them interpreted: LDS
 * frames, metering, WB_JIT=0, or a compile failure, whose message WasmEdge_BatchGetLastError
 * then returns until the next error). Results never depend on it. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetCompiledRuns(const WasmEdge_BatchContext *Cxt);

/* The execution engine the context runs, for reports (DESIGN.md "Execution engines"):
 * "<core>/<frames>", core one of "compiled-runs" (with "+simt" / "+trip" for the
 * scheduling inside them), "threaded-core" (the hand-written handlers, no compiled runs),
 * "compiled-step"; frames "vgpr-frames", "lds-frames" or "hbm-frames"; "+metered" when the
 * context meters gas. A context that wanted compiled runs and got none (a compile failure)
 * says "threaded-core (compiled runs failed)". Valid until the next call on the context;
 * "" for NULL. Results never depend on it. */
WASMEDGE_BATCH_API const char *WasmEdge_BatchGetEngine(const WasmEdge_BatchContext *Cxt);

/* The interleave granule in use, in bytes (WasmEdge_BatchConfigure::MemoryGranule).
 * Layout only: results never depend on it. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetMemoryGranule(const WasmEdge_BatchContext *Cxt);

/* Pages of every instance's memory in the reserved layout, which every execution path
 * addresses directly (pages past it come from pool rows through a page table). It starts at
 * MemoryReservePages (or the module's choice) and, at a BatchReset after a run whose
 * instances grew past it, takes the largest memory they reached (within 3/4 of the device
 * memory, and MemoryPoolBytes past the initial layout). Layout only: results never depend
 * on it. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetReservedPages(const WasmEdge_BatchContext *Cxt);
/* Pages every instance has reserved for memory MemIdx >= 1 (MultiMemories): memory.grow on
 * it returns -1 past them (0 for an index the module does not have). */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetExtraMemoryPages(const WasmEdge_BatchContext *Cxt,
                                                              uint32_t MemIdx);

/* Hash of every instance's final linear memory 0 (definition in DESIGN.md; the oracle
 * computes the same function). Hashes: [NumInstances]. */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchMemoryHash(WasmEdge_BatchContext *Cxt,
                                                            uint64_t *Hashes);
/* Copy Len bytes of instance Inst's linear memory starting at Off into Dst
 * (MemoryOutOfBounds 0x88 if outside its current size). */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchGetMemory(WasmEdge_BatchContext *Cxt,
                                                           uint32_t Inst, uint32_t Off,
                                                           uint8_t *Dst, uint32_t Len);
/* Write Len bytes into instance Inst's linear memory at Off (0x88 if outside it). */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchSetMemory(WasmEdge_BatchContext *Cxt,
                                                           uint32_t Inst, uint32_t Off,
                                                           const uint8_t *Src, uint32_t Len);
/* Bulk transfer: linear memory 0 of EVERY instance in one call -- the batched form of
 * WasmEdge_MemoryInstanceSetData / GetData (wasmedge.h:2552-2569), which the reference has
 * once per VM. Instance i moves len_i = Lens ? Lens[i] : Len bytes between row i of a
 * [NumInstances][Stride] byte buffer (byte i * Stride onward) and its memory, starting at
 * Offset + (Offsets ? Offsets[i] : 0), computed in 64 bits (a guest allocator returns a
 * different pointer per instance: Offsets would come from a previous run's results).
 * Offsets, Lens and PerInstance are host arrays [NumInstances], each may be NULL.
 *
 * Per instance, the reference's bound check (include/runtime/instance/memory.h:74-78): a
 * range that ends past the instance's current size gives PerInstance[i] = MemoryOutOfBounds
 * (0x88) and moves nothing of that instance -- its memory and its row of Dst stay as they
 * are; otherwise PerInstance[i] = 0 (also for len_i = 0 with the start within the size).
 * A read leaves the bytes of a row past len_i untouched. The call-level result is 0 even
 * when instances are out of bounds. Call-level failures, nothing moved: NULL context, NULL
 * Src / Dst with Len != 0, Stride < Len or some Lens[i] > Len give WrongVMWorkflow (0x04); a
 * module without a memory gives 0x88, as WasmEdge_BatchGetMemory does for any range.
 *
 * The call returns when the transfer is complete; it orders after a BatchReset that did
 * not wait (KernelSeconds NULL). Writes persist until BatchReset, like
 * WasmEdge_BatchSetMemory. Not to be called from inside a host function.
 *
 * The Device variants take Src / Dst as a device pointer to a buffer on the context's
 * device (for a torch tensor, its data_ptr): the rows never cross the host. The CALLER makes
 * sure that whatever produced the buffer has finished before the call (synchronise the
 * stream that wrote it); the library synchronises its own stream before it returns. On a
 * multi-device context one device buffer cannot serve several devices: they fail with
 * RuntimeError (0x02) and a WasmEdge_BatchGetLastError message; the host variants slice
 * Offsets, Lens and the rows by the placement and gather PerInstance in instance order. */
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchWriteMemories(WasmEdge_BatchContext *Cxt, const uint32_t *Offsets, uint32_t Offset,
                            const uint32_t *Lens, uint32_t Len, const uint8_t *Src,
                            uint64_t Stride, uint8_t *PerInstance);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchReadMemories(WasmEdge_BatchContext *Cxt, const uint32_t *Offsets, uint32_t Offset,
                           const uint32_t *Lens, uint32_t Len, uint8_t *Dst, uint64_t Stride,
                           uint8_t *PerInstance);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchWriteMemoriesDevice(WasmEdge_BatchContext *Cxt, const uint32_t *Offsets,
                                  uint32_t Offset, const uint32_t *Lens, uint32_t Len,
                                  const uint8_t *Src, uint64_t Stride, uint8_t *PerInstance);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchReadMemoriesDevice(WasmEdge_BatchContext *Cxt, const uint32_t *Offsets,
                                 uint32_t Offset, const uint32_t *Lens, uint32_t Len, uint8_t *Dst,
                                 uint64_t Stride, uint8_t *PerInstance);
/* Device-resident spans: the Device variants above with every instance's own offset and length
 * read on the device, so that the pointer an instance's own run returned never crosses the
 * host. Spans use the slot form of WasmEdge_BatchResultsDevice: instance i's own offset is the
 * low 32 bits of OffsetSlots[i * OffsetStride], its length len_i the low 32 bits of
 * LenSlots[i * LenStride]; the upper 32 bits are ignored, as BatchSetArgsDevice ignores them
 * for an i32. A column of a results buffer is passed as it lies: a pointer to the column's
 * first slot plus the row stride, in slots. NULL OffsetSlots: offset 0; NULL LenSlots: Len.
 *
 * Per instance exactly as the Device variants: the start is Offset + its own offset, computed
 * in 64 bits; a range that ends past the instance's current size gives MemoryOutOfBounds
 * (0x88) and moves nothing of that instance, neither its memory nor its row; status 0
 * otherwise, also for len_i = 0 with the start within the size; a read leaves the bytes of a
 * row past len_i untouched; writes persist until BatchReset. PerInstance is a DEVICE array
 * [NumInstances] (NULL: no status bytes exist anywhere); *NumOutOfBounds (host, may be NULL)
 * receives the number of instances given 0x88, so that a caller notices trouble without
 * copying NumInstances bytes. Per call the host reads back a few words and no per-instance
 * array; the library allocates nothing on the device after the context's first such call.
 *
 * Call-level failures, nothing moved -- the caller's rows, status bytes and memory stay as they
 * were -- and a WasmEdge_BatchGetLastError message: WrongVMWorkflow (0x04) for a NULL context,
 * NULL Src / Dst with Len != 0, Stride < Len, a slot pointer that is not 8-byte aligned, a
 * non-NULL slot pointer with stride 0, or some len_i > Len (found on the device; the message
 * names the lowest such i); 0x88 for a module without a memory; RuntimeError (0x02) for a
 * multi-device context, or a rows / slots / status buffer that this HIP runtime knows not to be
 * on the context's device or to be too short for NumInstances entries.
 *
 * Ordering as for the Device variants: the call orders after a BatchReset that did not wait,
 * the CALLER synchronises whatever produced the buffers, the library synchronises its own
 * stream before it returns. Not to be called from inside a host function. */
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchWriteMemoriesSpansDevice(
    WasmEdge_BatchContext *Cxt, const uint64_t *OffsetSlots, uint64_t OffsetStride, uint32_t Offset,
    const uint64_t *LenSlots, uint64_t LenStride, uint32_t Len, const uint8_t *Src, uint64_t Stride,
    uint8_t *PerInstance, uint32_t *NumOutOfBounds);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchReadMemoriesSpansDevice(
    WasmEdge_BatchContext *Cxt, const uint64_t *OffsetSlots, uint64_t OffsetStride, uint32_t Offset,
    const uint64_t *LenSlots, uint64_t LenStride, uint32_t Len, uint8_t *Dst, uint64_t Stride,
    uint8_t *PerInstance, uint32_t *NumOutOfBounds);
/* Waves (of 64 instances) of the last spans transfer that moved their bytes through the tiled
 * path: every instance of the wave that moved bytes started at one 4-byte aligned address, with
 * the rows' buffer and Stride 4-byte aligned too (DESIGN.md "Device-resident spans"). 0 for
 * NULL and before any such call. A report: results never depend on it. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetLastSpansTiledWaves(const WasmEdge_BatchContext *Cxt);
/* Instance snapshots: the state of EVERY instance as it stands between runs, held on the
 * device, and a restore that starts instance i from the captured state of instance SrcOf[i]
 * (SrcOf NULL: from its own) -- rewind after each try, fork, broadcast, survivor selection.
 * The reference has no counterpart (one VM is one instance; it would instantiate N VMs and
 * run their setup again). A restored instance continues exactly as its source would have.
 *
 * Captured and restored: memory 0 (contents, size and write mark of every instance),
 * memories 1..7 and their sizes, the globals, the per-instance tables with their sizes and
 * dropped element segments, the dropped data segments, the instantiation status, the gas
 * total (WasmEdge_BatchGetTotalCosts) and the built-in WASI state of every instance (captured
 * stdout / stderr, exit code, fd table, generator and clock counters; mapped through SrcOf,
 * except that an instance keeps its own index and its own args).
 * Not captured by SnapshotCreate: frames and the call stack (such a snapshot is taken
 * between runs, when no instance is parked at a host function; for a suspended invocation
 * see SnapshotCreateSuspended below), staged arguments and calls, the last run's results
 * (after a restore WasmEdge_BatchResults fails as after a BatchReset, until the next run),
 * externref handles (they live as long as the context) and the memory layout, which a
 * restore neither changes nor depends on: a snapshot stays valid when the granule, the
 * reserved pages or the table capacities changed since. The start function does not run
 * again.
 *
 * SnapshotCreate returns NULL and sets *Res on failure: WrongVMWorkflow (0x04) for a NULL
 * context; RuntimeError (0x02) with a WasmEdge_BatchGetLastError message when device memory
 * runs out, or when instances hold pages past the reserved layout and it cannot grow to take
 * them (the context stays usable). GetBytes: the device memory the snapshot holds, in bytes
 * -- what the instances wrote, not the size of their memories.
 *
 * SnapshotRestore fails, with all state unchanged, with WrongVMWorkflow (0x04) for a NULL
 * context or snapshot, a snapshot of another context (or of one deleted since) or some
 * SrcOf[i] >= NumInstances, and with RuntimeError (0x02) and a message for a non-NULL SrcOf on
 * a multi-device context (rows cannot cross devices; NULL works there). *KernelSeconds (may
 * be NULL) = the device time of the restore; NULL: no host synchronisation, the next launch
 * orders after it, as with BatchReset. A snapshot outlives BatchReset and other restores and
 * may be restored any number of times; SnapshotDelete is safe before or after BatchDelete of
 * its context. Not to be called from inside a host function.
 *
 * SnapshotCreateSuspended: everything SnapshotCreate captures plus the suspended invocation
 * of a Resumable context (resumable runs, above) -- every instance's frame, call stack and
 * resume point, its status, instruction count and result row, and the invocation itself
 * (the function or the call vector, the result types). Legal only while an invocation is
 * live: after a completed BatchRun / BatchResume and before anything that ends it; otherwise
 * (NULL, a context that is not Resumable, before any BatchRun, after BatchReset / SetArgs /
 * SetCalls / a plain restore) NULL with WrongVMWorkflow (0x04). Zero suspended instances is
 * legal. Device-memory failures as for SnapshotCreate. SnapshotGetSuspendedCount: the
 * suspended instances the snapshot holds; 0 for NULL and for a snapshot without an
 * invocation; a multi-device snapshot sums its shards.
 *
 * SnapshotRestore of such a snapshot restores the instance state as above and then
 * reinstates the invocation: instance i continues, at the next BatchResume, exactly as
 * instance SrcOf[i] would have from the capture; an instance whose source had finished,
 * trapped or sat the call out is final with the source's status, count and returns and does
 * not run. BatchGetSuspendedCount then reports the suspended sources under the map,
 * BatchResults works at once and returns the rows as they stood at the capture (through
 * SrcOf, as do BatchGetReturnLens and the result types of a call vector), and InstrCounts
 * continue cumulatively, so the caller goes on with the same k * slice. It is legal whatever
 * the context did since the capture (BatchReset, runs of other exports, SetCalls, other
 * restores); a call stack that BatchReset shrank since grows back first (RuntimeError 0x02
 * with a message when it cannot, all state unchanged). Reset, SetArgs, SetCalls, Run and a
 * restore of a snapshot without an invocation end it as usual. The staged arguments are not
 * captured: when the restore maps instances (SrcOf) or the context staged other arguments
 * since the capture, a BatchRun needs SetArgs / SetCalls first (WrongVMWorkflow otherwise).
 *
 * SnapshotRestoreSelected: a restore that leaves some instances alone -- "reset the finished
 * environments, step the others". SrcOf is [NumInstances] and must not be NULL (for "every
 * instance from itself" there is SnapshotRestore). SrcOf[i] == WASMEDGE_BATCH_SNAPSHOT_KEEP:
 * instance i keeps everything a snapshot would have overwritten -- memory 0 with its size and
 * write mark, memories 1..7 and their sizes, its globals, its tables with their sizes and
 * dropped element segments, its dropped data segments, its instantiation status, its gas total
 * and its built-in WASI state. Any other entry means what it means for SnapshotRestore.
 * *NumRestored (may be NULL) = the instances that were not kept. (SnapshotRestore keeps its
 * contract to the letter: 0xFFFFFFFF there is an instance past NumInstances, 0x04.) For the
 * call as a whole it is a SnapshotRestore: the last run's results are gone, a live suspended
 * invocation of the context ends (kept instances are written "not parked" with the others, so
 * the next BatchRun starts them cleanly), staged arguments stay, the layout neither changes
 * nor matters. Failures, with all state unchanged: WrongVMWorkflow (0x04) for a NULL context,
 * snapshot or map, a snapshot of another context, an entry that is neither KEEP nor below
 * NumInstances, and for a map with a KEEP together with a snapshot that holds an invocation
 * (SnapshotCreateSuspended): which invocation a kept instance would then belong to is not
 * defined here. A map without KEEP on such a snapshot behaves exactly as SnapshotRestore.
 * RuntimeError (0x02) with a message when a kept instance holds pages past the reserved layout
 * and the layout cannot grow to take them (as SnapshotCreate; the context stays usable), and
 * on a multi-device context for a map with an entry that is neither KEEP nor i (nothing may
 * cross a device; a map of KEEP and i entries is legal there; the pool-row step runs on every
 * shard before the first is restored, while a device error in the middle may leave earlier
 * shards restored, as with SnapshotRestore).
 *
 * SnapshotRestoreSelectedDevice: the same from a map in device memory (a selection computed
 * on the device from statuses or results that never left it). The caller synchronises
 * whatever produced SrcOfDevice. A buffer this HIP runtime allocated must lie on the
 * context's device and hold NumInstances words, else RuntimeError (0x02); so is any call on a
 * multi-device context. The map is validated and the restore planned by a kernel; the call
 * synchronises once before the restore's kernels, to read that kernel's summary -- an invalid
 * map (0x04) leaves the context as it was --, and with KernelSeconds NULL does not wait after
 * them. For a snapshot that holds WASI state or an invocation the map is read back once
 * (NumInstances * 4 bytes) and the call is SnapshotRestoreSelected. */
#define WASMEDGE_BATCH_SNAPSHOT_KEEP 0xFFFFFFFFu
typedef struct WasmEdge_BatchSnapshot WasmEdge_BatchSnapshot;
WASMEDGE_BATCH_API WasmEdge_BatchSnapshot *WasmEdge_BatchSnapshotCreate(WasmEdge_BatchContext *Cxt,
                                                                        WasmEdge_Result *Res);
WASMEDGE_BATCH_API WasmEdge_BatchSnapshot *WasmEdge_BatchSnapshotCreateSuspended(WasmEdge_BatchContext *Cxt,
                                                                                 WasmEdge_Result *Res);
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchSnapshotGetSuspendedCount(const WasmEdge_BatchSnapshot *Snap);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSnapshotRestore(WasmEdge_BatchContext *Cxt, const WasmEdge_BatchSnapshot *Snap,
                              const uint32_t *SrcOf, double *KernelSeconds);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSnapshotRestoreSelected(WasmEdge_BatchContext *Cxt, const WasmEdge_BatchSnapshot *Snap,
                                      const uint32_t *SrcOf, uint32_t *NumRestored, double *KernelSeconds);
WASMEDGE_BATCH_API WasmEdge_Result
WasmEdge_BatchSnapshotRestoreSelectedDevice(WasmEdge_BatchContext *Cxt, const WasmEdge_BatchSnapshot *Snap,
                                            const uint32_t *SrcOfDevice, uint32_t *NumRestored,
                                            double *KernelSeconds);
WASMEDGE_BATCH_API uint64_t WasmEdge_BatchSnapshotGetBytes(const WasmEdge_BatchSnapshot *Snap);
WASMEDGE_BATCH_API void WasmEdge_BatchSnapshotDelete(WasmEdge_BatchSnapshot *Snap);
/* Exported tables and globals of one instance, by export name (the batched form of
 * WasmEdge_StoreFindTable/FindGlobal + WasmEdge_TableInstanceGetData/SetData/GetSize,
 * lib/api/wasmedge.cpp:2099-2139, and WasmEdge_GlobalInstanceGetValue/SetValue,
 * :2273-2295). Inst = WASMEDGE_BATCH_ALL_INSTANCES writes every instance. Reference
 * values: a funcref is the module's function index; an externref is any 64-bit host value
 * (a pointer, as WasmEdge_ValueGenExternRef makes, wasmedge.h:254,318), given back
 * unchanged wherever it leaves the batch (results, host-function arguments, table and
 * global reads); null is 0xFFFFFFFF for both. (On the device refs are 32-bit: a value
 * from 2^31 up is carried as a handle the context interns.) TableGetData/SetData: TableOutOfBounds (0x87) past the instance's table
 * size, RefTypeMismatch (0x8E) for a value of the wrong reference type. GlobalSetValue
 * ignores a constant global or a value of another type, as the reference does. An
 * unknown export name gives FuncNotFound (0x05). Writes persist until BatchReset. */
#define WASMEDGE_BATCH_ALL_INSTANCES 0xFFFFFFFFu
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchTableGetSize(WasmEdge_BatchContext *Cxt,
                                                              const WasmEdge_String TableName,
                                                              uint32_t Inst, uint32_t *Size);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchTableGetData(WasmEdge_BatchContext *Cxt,
                                                              const WasmEdge_String TableName,
                                                              uint32_t Inst, WasmEdge_Value *Data,
                                                              uint32_t Offset);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchTableSetData(WasmEdge_BatchContext *Cxt,
                                                              const WasmEdge_String TableName,
                                                              uint32_t Inst, WasmEdge_Value Data,
                                                              uint32_t Offset);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchGlobalGetValue(WasmEdge_BatchContext *Cxt,
                                                                const WasmEdge_String GlobalName,
                                                                uint32_t Inst, WasmEdge_Value *Value);
WASMEDGE_BATCH_API WasmEdge_Result WasmEdge_BatchGlobalSetValue(WasmEdge_BatchContext *Cxt,
                                                                const WasmEdge_String GlobalName,
                                                                uint32_t Inst, WasmEdge_Value Value);
/* Current page count of instance Inst's memory. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetMemoryPages(WasmEdge_BatchContext *Cxt,
                                                         uint32_t Inst);
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetInstanceCount(const WasmEdge_BatchContext *Cxt);
/* Hash of the sources this library was built from (wasmedge_amd/csrc/srchash.py): lets a
 * caller check that the library it loaded matches the checked-out tree (the batched form
 * of the reference's WasmEdge_VersionGet, wasmedge.h). */
WASMEDGE_BATCH_API const char *WasmEdge_BatchGetBuildHash(void);
/* Human-readable description of the last failure on this context (or of the last
 * failed BatchCreate when Cxt is NULL). */
WASMEDGE_BATCH_API const char *WasmEdge_BatchGetLastError(const WasmEdge_BatchContext *Cxt);
/* Number of device instructions and max wasm instructions folded into one dispatch. */
WASMEDGE_BATCH_API uint32_t WasmEdge_BatchGetCodeSize(const WasmEdge_BatchContext *Cxt);
WASMEDGE_BATCH_API void WasmEdge_BatchDelete(WasmEdge_BatchContext *Cxt);

#ifdef __cplusplus
}
#endif
#endif
