"""Python host mirror of the batched C ABI (include/wasmedge_batch.h) over ctypes.

Mirrors the reference VM/C-API flow (lib/vm/vm.cpp, include/api/wasmedge/wasmedge.h):
load -> validate -> instantiate -> execute, but for N instances at once.  The product
path is the HIP library `libwasmedge_batch.so`; there is no CPU fallback -- if the library
or a GPU is missing, construction raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WB_BATCH_LIB selects a profiling variant (libwasmedge_batch_stats.so, tools/ only)
LIB_PATH = os.environ.get("WB_BATCH_LIB") or os.path.join(_HERE, "libwasmedge_batch.so")

# valtypes (include/api/wasmedge/enum_types.h)
I32, I64, F32, F64, V128, FUNCREF, EXTERNREF = 0x7F, 0x7E, 0x7D, 0x7C, 0x7B, 0x70, 0x6F

# WasmEdge_Value: {uint128_t Value; enum WasmEdge_ValType Type;} -> 32 bytes (16-aligned)
VALUE_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("type", "<u4"), ("pad", "<u4", (3,))])

# per-instance status codes (reference ErrCodes, include/common/enum.inc:717-745)
STATUS_NAMES = {0x00: "ok", 0x07: "interrupted", 0x84: "integer divide by zero",
                0x85: "integer overflow", 0x86: "invalid conversion to integer",
                0x87: "out of bounds table access", 0x88: "out of bounds memory access",
                0x89: "unreachable", 0x8A: "uninitialized element", 0x8B: "undefined element",
                0x8C: "indirect call type mismatch", 0xB0: "call stack exhausted",
                0xB1: "host call (yield path not implemented)"}


ALL_INSTANCES = 0xFFFFFFFF
NO_CALL = 0xFFFFFFFF    # WASMEDGE_BATCH_NO_CALL: the instance sits a set_calls run out
KEEP = 0xFFFFFFFF       # WASMEDGE_BATCH_SNAPSHOT_KEEP: restore_selected leaves the instance alone
REF_NULL = 0xFFFFFFFF   # null funcref / externref on the device (32-bit references)


class _Value(ctypes.Structure):
    """WasmEdge_Value passed by value: uint128 as two u64 words, then the type."""
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64), ("type", ctypes.c_uint32),
                ("pad", ctypes.c_uint32 * 3)]

    @classmethod
    def make(cls, value, vtype):
        v = int(value) & ((1 << 128) - 1)
        return cls(v & 0xFFFFFFFFFFFFFFFF, v >> 64, vtype)

    def int(self):
        return self.lo | (self.hi << 64)


class WasmEdgeError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("WasmEdge_Result 0x%02x %s" % (code, msg))
        self.code = code


class _Conf(ctypes.Structure):
    _fields_ = [("MaxMemoryPage", ctypes.c_uint32), ("CallStackCells", ctypes.c_uint32),
                ("MaxSteps", ctypes.c_uint64), ("TimeLimitSeconds", ctypes.c_double),
                ("DeviceOrdinal", ctypes.c_int32), ("CostLimit", ctypes.c_uint64),
                ("HostThreads", ctypes.c_uint32), ("CostTable", ctypes.c_void_p),
                ("CostTableLen", ctypes.c_uint32), ("MemoryGranule", ctypes.c_uint32),
                ("TailCall", ctypes.c_uint32), ("MemoryReservePages", ctypes.c_uint32),
                ("MemoryPoolBytes", ctypes.c_uint64), ("Devices", ctypes.POINTER(ctypes.c_int32)),
                ("DeviceCount", ctypes.c_uint32), ("Partition", ctypes.c_uint32),
                ("MultiMemories", ctypes.c_uint32), ("ExtraMemoryReservePages", ctypes.c_uint32),
                ("CallStackMaxBytes", ctypes.c_uint64), ("Resumable", ctypes.c_uint32)]

PARTITION_BLOCKS, PARTITION_INTERLEAVE = 0, 1


def placement(n, device_count, partition, inst):
    """(shard, lane) of instance `inst` in an n-instance batch over device_count devices
    (WasmEdge_BatchPlacement; no device needed)."""
    g, l = ctypes.c_uint32(), ctypes.c_uint32()
    r = lib().WasmEdge_BatchPlacement(n, device_count, partition, inst, ctypes.byref(g), ctypes.byref(l))
    if r.Code:
        raise WasmEdgeError(r.Code, "placement")
    return g.value, l.value


class _String(ctypes.Structure):
    _fields_ = [("Length", ctypes.c_uint32), ("Buf", ctypes.c_char_p)]


class _Import(ctypes.Structure):
    """WasmEdge_BatchImport: a provided table / memory / global."""
    _fields_ = [("ModuleName", _String), ("ExternalName", _String), ("Kind", ctypes.c_uint32),
                ("Min", ctypes.c_uint32), ("Max", ctypes.c_uint32), ("HasMax", ctypes.c_uint32),
                ("Type", ctypes.c_uint32), ("Mutable", ctypes.c_uint32),
                ("_align", ctypes.c_uint32 * 2),   # WasmEdge_Value is 16-byte aligned (uint128)
                ("Value", _Value)]


class _Result(ctypes.Structure):
    _fields_ = [("Code", ctypes.c_uint8)]


_lib = None

# WasmEdge_BatchHostFunc_t: WasmEdge_Result(void *Data, MemCxt *, const Value *, Value *).
# WasmEdge_Result is a one-byte struct, returned in a register exactly like a uint8_t.
HOST_FUNC = ctypes.CFUNCTYPE(ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p)


class HostMemory:
    """The calling instance's linear memory inside a host function
    (WasmEdge_BatchMemoryGetData / SetData)."""

    def __init__(self, handle):
        self._h = handle
        self.instance = lib().WasmEdge_BatchMemoryGetInstance(handle)

    def read(self, off, length):
        buf = ctypes.create_string_buffer(max(length, 1))
        r = lib().WasmEdge_BatchMemoryGetData(self._h, buf, off, length)
        if r.Code:
            raise WasmEdgeError(r.Code, "memory read")
        return buf.raw[:length]

    def write(self, off, data):
        r = lib().WasmEdge_BatchMemorySetData(self._h, bytes(data), off, len(data))
        if r.Code:
            raise WasmEdgeError(r.Code, "memory write")


def lib():
    """Load the HIP library (raises if it was not built -- no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("libwasmedge_batch.so not built: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.WasmEdge_BatchCreate.restype = vp
        L.WasmEdge_BatchCreate.argtypes = [ctypes.POINTER(_Conf), ctypes.c_char_p, u32, u32,
                                           ctypes.POINTER(_Result)]
        L.WasmEdge_BatchCreateWithImports.restype = vp
        L.WasmEdge_BatchCreateWithImports.argtypes = [ctypes.POINTER(_Conf), ctypes.c_char_p, u32, u32,
                                                      ctypes.POINTER(_Import), u32,
                                                      ctypes.POINTER(_Result)]
        for name, args in [
            ("WasmEdge_BatchExecute", [vp, _String, vp, u32, vp, u32, vp, vp]),
            ("WasmEdge_BatchSetArgs", [vp, _String, vp, u32]),
            ("WasmEdge_BatchReset", [vp, ctypes.POINTER(ctypes.c_double)]),
            ("WasmEdge_BatchRun", [vp, ctypes.POINTER(ctypes.c_double)]),
            ("WasmEdge_BatchResume", [vp, u64, ctypes.POINTER(ctypes.c_double)]),
            ("WasmEdge_BatchResults", [vp, vp, u32, vp, vp]),
            ("WasmEdge_BatchMemoryHash", [vp, vp]),
            ("WasmEdge_BatchGetMemory", [vp, u32, u32, vp, u32]),
            ("WasmEdge_BatchSetCalls", [vp, ctypes.POINTER(_String), u32, vp, vp, u32, vp]),
            ("WasmEdge_BatchExecuteCalls", [vp, ctypes.POINTER(_String), u32, vp, vp, u32, vp,
                                            vp, u32, vp, vp, vp]),
            ("WasmEdge_BatchGetReturnLens", [vp, vp]),
            ("WasmEdge_BatchWriteMemories", [vp, vp, u32, vp, u32, vp, u64, vp]),
            ("WasmEdge_BatchReadMemories", [vp, vp, u32, vp, u32, vp, u64, vp]),
            ("WasmEdge_BatchWriteMemoriesDevice", [vp, vp, u32, vp, u32, vp, u64, vp]),
            ("WasmEdge_BatchReadMemoriesDevice", [vp, vp, u32, vp, u32, vp, u64, vp]),
            ("WasmEdge_BatchWriteMemoriesSpansDevice", [vp, vp, u64, u32, vp, u64, u32, vp, u64, vp, vp]),
            ("WasmEdge_BatchReadMemoriesSpansDevice", [vp, vp, u64, u32, vp, u64, u32, vp, u64, vp, vp]),
            ("WasmEdge_BatchSetArgsDevice", [vp, _String, vp, u32, vp, u64]),
            ("WasmEdge_BatchResultsDevice", [vp, vp, u32, u64, vp, vp]),
            ("WasmEdge_BatchSetCallsDevice", [vp, ctypes.POINTER(_String), u32, vp, vp, vp, vp, u64]),
            ("WasmEdge_BatchCallsResultsDevice", [vp, vp, u32, u64, vp, vp, vp]),
        ]:
            f = getattr(L, name)
            f.restype = _Result
            f.argtypes = args
        L.WasmEdge_BatchGetMemoryPages.restype = u32
        L.WasmEdge_BatchGetMemoryPages.argtypes = [vp, u32]
        L.WasmEdge_BatchGetSuspendedCount.restype = u32
        L.WasmEdge_BatchGetSuspendedCount.argtypes = [vp]
        L.WasmEdge_BatchGetInstanceCount.restype = u32
        L.WasmEdge_BatchGetInstanceCount.argtypes = [vp]
        L.WasmEdge_BatchGetCodeSize.restype = u32
        L.WasmEdge_BatchGetCodeSize.argtypes = [vp]
        L.WasmEdge_BatchGetLastError.restype = ctypes.c_char_p
        L.WasmEdge_BatchGetLastError.argtypes = [vp]
        L.WasmEdge_BatchDelete.restype = None
        L.WasmEdge_BatchDelete.argtypes = [vp]
        for name, args in [
            ("WasmEdge_BatchSetMemory", [vp, u32, u32, ctypes.c_char_p, u32]),
            ("WasmEdge_BatchAddHostFunction", [vp, _String, _String, HOST_FUNC, vp]),
            ("WasmEdge_BatchAddHostFunctionWithCost", [vp, _String, _String, HOST_FUNC, vp, u64]),
            ("WasmEdge_BatchMemoryGetData", [vp, vp, u32, u32]),
            ("WasmEdge_BatchMemorySetData", [vp, ctypes.c_char_p, u32, u32]),
        ]:
            f = getattr(L, name)
            f.restype = _Result
            f.argtypes = args
        for name, args in [
            ("WasmEdge_BatchTableGetSize", [vp, _String, u32, ctypes.POINTER(u32)]),
            ("WasmEdge_BatchTableGetData", [vp, _String, u32, ctypes.POINTER(_Value), u32]),
            ("WasmEdge_BatchTableSetData", [vp, _String, u32, _Value, u32]),
            ("WasmEdge_BatchGlobalGetValue", [vp, _String, u32, ctypes.POINTER(_Value)]),
            ("WasmEdge_BatchGlobalSetValue", [vp, _String, u32, _Value]),
        ]:
            f = getattr(L, name)
            f.restype = _Result
            f.argtypes = args
        L.WasmEdge_BatchPlacement.restype = _Result
        L.WasmEdge_BatchPlacement.argtypes = [u32, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.WasmEdge_BatchInterrupt.restype = None
        L.WasmEdge_BatchInterrupt.argtypes = [vp]
        L.WasmEdge_BatchMemoryGetInstance.restype = u32
        L.WasmEdge_BatchMemoryGetInstance.argtypes = [vp]
        cpp = ctypes.POINTER(ctypes.c_char_p)
        L.WasmEdge_BatchGetTotalCosts.restype = _Result
        L.WasmEdge_BatchGetTotalCosts.argtypes = [vp, vp]
        L.WasmEdge_BatchInitWASI.restype = _Result
        L.WasmEdge_BatchInitWASI.argtypes = [vp, cpp, u32, cpp, u32]
        L.WasmEdge_BatchInitWASIWithPreopens.restype = _Result
        L.WasmEdge_BatchInitWASIWithPreopens.argtypes = [vp, cpp, u32, cpp, u32, cpp, u32]
        L.WasmEdge_BatchWASISetDeterministic.restype = _Result
        L.WasmEdge_BatchWASISetDeterministic.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64]
        L.WasmEdge_BatchWASISetInstanceArgs.restype = _Result
        L.WasmEdge_BatchWASISetInstanceArgs.argtypes = [vp, u32, cpp, u32]
        L.WasmEdge_BatchWASIGetExitCode.restype = u32
        L.WasmEdge_BatchWASIGetExitCode.argtypes = [vp, u32]
        L.WasmEdge_BatchWASIGetOutput.restype = u32
        L.WasmEdge_BatchWASIGetOutput.argtypes = [vp, u32, u32, vp, u32]
        L.WasmEdge_BatchGetCompiledRuns.restype = u32
        L.WasmEdge_BatchGetCompiledRuns.argtypes = [vp]
        L.WasmEdge_BatchGetMemoryGranule.restype = u32
        L.WasmEdge_BatchGetMemoryGranule.argtypes = [vp]
        L.WasmEdge_BatchGetLastSpansTiledWaves.restype = u32
        L.WasmEdge_BatchGetLastSpansTiledWaves.argtypes = [vp]
        L.WasmEdge_BatchGetReservedPages.restype = u32
        L.WasmEdge_BatchGetReservedPages.argtypes = [vp]
        L.WasmEdge_BatchGetExtraMemoryPages.restype = u32
        L.WasmEdge_BatchGetExtraMemoryPages.argtypes = [vp, u32]
        L.WasmEdge_BatchGetEngine.restype = ctypes.c_char_p
        L.WasmEdge_BatchGetEngine.argtypes = [vp]
        L.WasmEdge_BatchSnapshotCreate.restype = vp
        L.WasmEdge_BatchSnapshotCreate.argtypes = [vp, ctypes.POINTER(_Result)]
        L.WasmEdge_BatchSnapshotCreateSuspended.restype = vp
        L.WasmEdge_BatchSnapshotCreateSuspended.argtypes = [vp, ctypes.POINTER(_Result)]
        L.WasmEdge_BatchSnapshotGetSuspendedCount.restype = ctypes.c_uint32
        L.WasmEdge_BatchSnapshotGetSuspendedCount.argtypes = [vp]
        L.WasmEdge_BatchSnapshotRestore.restype = _Result
        L.WasmEdge_BatchSnapshotRestore.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_double)]
        for f in (L.WasmEdge_BatchSnapshotRestoreSelected, L.WasmEdge_BatchSnapshotRestoreSelectedDevice):
            f.restype = _Result
            f.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)]
        L.WasmEdge_BatchSnapshotGetBytes.restype = u64
        L.WasmEdge_BatchSnapshotGetBytes.argtypes = [vp]
        L.WasmEdge_BatchSnapshotDelete.restype = None
        L.WasmEdge_BatchSnapshotDelete.argtypes = [vp]
        _lib = L
    return _lib


def make_values(rows, types):
    """rows: iterable of per-instance argument tuples (python ints, bit patterns for
    floats) or a numpy integer array [n, nparams]; types: list of valtypes."""
    if isinstance(rows, np.ndarray):
        arr = rows.reshape(rows.shape[0], -1)
        n = arr.shape[0]
        out = np.zeros((n, len(types)), VALUE_DTYPE)
        for k, t in enumerate(types):
            col = arr[:, k].astype(np.uint64) if arr.dtype.kind == "u" else \
                arr[:, k].astype(np.int64).view(np.uint64)
            if t in (I32, F32, FUNCREF):   # (an externref is any 64-bit host value)
                col = col & np.uint64(0xFFFFFFFF)
            out["lo"][:, k] = col
            out["type"][:, k] = t
        return out
    rows = list(rows)
    out = np.zeros((len(rows), len(types)), VALUE_DTYPE)
    for i, r in enumerate(rows):
        for k, t in enumerate(types):
            v = int(r[k]) & ((1 << 128) - 1)
            if t in (I32, F32, FUNCREF):
                v &= 0xFFFFFFFF
            elif t in (I64, F64, EXTERNREF):
                v &= (1 << 64) - 1
            out["lo"][i, k] = v & 0xFFFFFFFFFFFFFFFF
            out["hi"][i, k] = v >> 64
            out["type"][i, k] = t
    return out


def slots_of(types):
    """Width of a device row of these value types in 64-bit slots (set_args_tensor /
    results_tensor): one slot per value, two for a v128."""
    n = 0
    for t in types:
        if t not in (I32, I64, F32, F64, V128, FUNCREF, EXTERNREF):
            raise ValueError("0x%02x is not a value type" % t)
        n += 2 if t == V128 else 1
    return n


def call_names(funcs, types=None):
    """The host arguments of WasmEdge_BatchSetCallsDevice: (names, FuncNames array, ParamTypes
    pointer or None, ParamLens pointer or None, what has to stay alive for the call). types:
    None, or one list of value types per name."""
    funcs = list(funcs)
    if not all(isinstance(f, str) for f in funcs):
        raise ValueError("funcs must be export names")
    names = [f.encode() for f in funcs]
    arr = (_String * max(len(names), 1))(*[_String(len(b), b) for b in names])
    if types is None:
        return names, arr, None, None, (names, arr)
    types = [[int(x) for x in row] for row in types]
    if len(types) != len(funcs):
        raise ValueError("types must hold one list of value types per name")
    for row in types:
        slots_of(row)   # (ValueError for what is no value type)
    rows = [np.array(row, np.uint32) for row in types]
    ptrs = (ctypes.c_void_p * max(len(rows), 1))(*[r.ctypes.data if len(r) else None for r in rows])
    lens = np.array([len(r) for r in rows] + [0], np.uint32)
    return names, arr, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data, (names, arr, rows, ptrs, lens)


class BatchContext:
    """N instances of one module on one GPU (WasmEdge_BatchContext)."""

    def __init__(self, wasm, n, max_memory_page=0, call_stack_cells=0, max_steps=0,
                 time_limit=0.0, device=-1, cost_limit=0, host_threads=0, cost_table=None,
                 memory_granule=0, imports=None, tail_call=False, memory_reserve_pages=0,
                 memory_pool_bytes=0, devices=None, partition=PARTITION_BLOCKS, multi_memory=False,
                 extra_memory_reserve_pages=0, call_stack_max_bytes=0, resumable=False):
        """cost_table: gas cost per OpCode (list; missing entries 0), None = unit costs;
        metering is on when cost_limit > 0. max_memory_page 0 = the reference's default
        page limit (65536); memory_reserve_pages / memory_pool_bytes: the device layout of
        grown memory (WasmEdge_BatchConfigure). devices: a list of HIP ordinals (repeats
        allowed) to spread the instances over from this process, by `partition`. resumable:
        instances that end a run with 0x07 are suspended and resume() continues them."""
        L = lib()
        tab = None
        if cost_table is not None:
            tab = np.ascontiguousarray(cost_table, np.uint64)
        conf = _Conf(max_memory_page, call_stack_cells, max_steps, time_limit, device, cost_limit,
                     host_threads, tab.ctypes.data if tab is not None and len(tab) else None,
                     len(tab) if tab is not None else 0, memory_granule, 1 if tail_call else 0,
                     memory_reserve_pages, memory_pool_bytes)
        conf.MultiMemories = 1 if multi_memory else 0
        conf.ExtraMemoryReservePages = extra_memory_reserve_pages
        conf.CallStackMaxBytes = call_stack_max_bytes
        conf.Resumable = 1 if resumable else 0
        if devices is not None and len(devices) == 1:
            conf.DeviceOrdinal = devices[0]
        if devices is not None and len(devices) > 1:
            self._devices = (ctypes.c_int32 * len(devices))(*devices)
            conf.Devices = self._devices
            conf.DeviceCount = len(devices)
            conf.Partition = partition
        res = _Result(0)
        imps = imports or []
        arr = (_Import * max(1, len(imps)))()
        self._import_names = []
        for k, i in enumerate(imps):
            mod, nm = i["module"].encode(), i["name"].encode()
            self._import_names += [mod, nm]
            mx = i.get("max")
            arr[k] = _Import(_String(len(mod), mod), _String(len(nm), nm), i["kind"], i.get("min", 0),
                             mx or 0, 0 if mx is None else 1, i.get("type", 0),
                             1 if i.get("mut") else 0, (ctypes.c_uint32 * 2)(),
                             _Value.make(i.get("value", 0), i.get("type", 0)))
        self._h = L.WasmEdge_BatchCreateWithImports(ctypes.byref(conf), bytes(wasm), len(wasm), n,
                                                    arr, len(imps), ctypes.byref(res))
        if not self._h:
            raise WasmEdgeError(res.Code, L.WasmEdge_BatchGetLastError(None).decode())
        self.n = n
        self.func = None

    def close(self):
        if getattr(self, "_h", None):
            lib().WasmEdge_BatchDelete(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, r):
        if r.Code:
            raise WasmEdgeError(r.Code, lib().WasmEdge_BatchGetLastError(self._h).decode())

    @staticmethod
    def _name(func):
        b = func.encode()
        return _String(len(b), b)

    def set_args(self, func, values):
        values = np.ascontiguousarray(values, VALUE_DTYPE)
        # WasmEdge_BatchSetArgs reads NumInstances rows: a shorter array would be read past
        if values.ndim != 2 or values.shape[0] != self.n:
            raise ValueError("values must be [%d instances][params], got shape %s"
                             % (self.n, values.shape))
        nparams = values.shape[1]
        self._check(lib().WasmEdge_BatchSetArgs(self._h, self._name(func),
                                                values.ctypes.data if values.size else None,
                                                nparams))
        self.func = func
        self._keep = values

    def reset(self, timed=True):
        """Re-instantiate every instance; returns the reset kernels' time (timed=False: no
        host synchronisation, returns 0 -- the next run orders after it on the stream)."""
        t = ctypes.c_double(0)
        self._check(lib().WasmEdge_BatchReset(self._h, ctypes.byref(t) if timed else None))
        return t.value

    def run(self):
        t = ctypes.c_double(0)
        self._check(lib().WasmEdge_BatchRun(self._h, ctypes.byref(t)))
        return t.value

    def resume(self, step_limit=0, timed=True):
        """Continue the suspended instances (status 0x07) of the last run() / resume() on a
        resumable context (WasmEdge_BatchResume). step_limit: the new cumulative instruction
        limit per instance, in the units of results()' counts (0: none). Returns the kernel
        time (timed=False: 0)."""
        t = ctypes.c_double(0)
        self._check(lib().WasmEdge_BatchResume(self._h, step_limit, ctypes.byref(t) if timed else None))
        return t.value

    def suspended(self):
        """Instances suspended after the last run() / resume() (WasmEdge_BatchGetSuspendedCount)."""
        return lib().WasmEdge_BatchGetSuspendedCount(self._h)

    def results(self, nret):
        rets = np.zeros((self.n, max(nret, 1)), VALUE_DTYPE)
        status = np.zeros(self.n, np.uint8)
        counts = np.zeros(self.n, np.uint64)
        self._check(lib().WasmEdge_BatchResults(self._h, rets.ctypes.data, nret,
                                                status.ctypes.data, counts.ctypes.data))
        return rets[:, :nret], status, counts

    def execute(self, func, values, nret):
        """Invoke `func` on every instance (WasmEdge_BatchExecute: state persists from
        the previous invocation; reset() re-instantiates). Returns (returns[n, nret]
        VALUE_DTYPE, status, counts)."""
        self.set_args(func, values)
        self.run()
        return self.results(nret)

    # per-instance calls (WasmEdge_BatchSetCalls / ExecuteCalls / GetReturnLens)
    def set_calls(self, funcs, func_of, rows):
        """Each instance its own export: funcs = the export names, func_of[i] = instance i's
        index into funcs or None (no call: it sits the run out with status 0), rows[i] = its
        arguments as (value, valtype) pairs (ints, bit patterns for floats). An unknown
        name gives that instance 0x05, arguments that do not match its function 0x83; run()
        and results(stride) then work as after set_args."""
        keep, args = self._pack_calls(funcs, func_of, rows)
        self._check(lib().WasmEdge_BatchSetCalls(self._h, *args))
        self.func = None
        self._keep = keep

    def _pack_calls(self, funcs, func_of, rows):
        if len(func_of) != self.n or len(rows) != self.n:
            raise ValueError("func_of and rows must have %d entries" % self.n)
        names = [f.encode() for f in funcs]
        arr = (_String * max(len(names), 1))(*[_String(len(b), b) for b in names])
        fo = np.array([NO_CALL if f is None else f for f in func_of], np.uint32)
        lens = np.array([len(r) for r in rows], np.uint32)
        stride = int(lens.max()) if self.n else 0
        vals = np.zeros((self.n, max(stride, 1)), VALUE_DTYPE)
        for i, r in enumerate(rows):
            for k, (v, t) in enumerate(r):
                v = int(v) & ((1 << 128) - 1)
                vals["lo"][i, k] = v & 0xFFFFFFFFFFFFFFFF
                vals["hi"][i, k] = v >> 64
                vals["type"][i, k] = t
        return (names, arr, fo, vals, lens), (arr, len(names), fo.ctypes.data,
                                              vals.ctypes.data if stride else None, stride,
                                              lens.ctypes.data)

    def return_lens(self):
        """Result count of each instance's function (0 where it did not run)."""
        lens = np.zeros(self.n, np.uint32)
        self._check(lib().WasmEdge_BatchGetReturnLens(self._h, lens.ctypes.data))
        return lens

    def execute_calls(self, funcs, func_of, rows, max_returns=8):
        """WasmEdge_BatchExecuteCalls (arguments as set_calls): (rets, status, counts),
        rets[i] = instance i's return values as python ints, as many as its function has
        (up to max_returns; none unless its status is 0)."""
        keep, args = self._pack_calls(funcs, func_of, rows)
        rets = np.zeros((self.n, max(max_returns, 1)), VALUE_DTYPE)
        lens = np.zeros(self.n, np.uint32)
        status = np.zeros(self.n, np.uint8)
        counts = np.zeros(self.n, np.uint64)
        self._check(lib().WasmEdge_BatchExecuteCalls(self._h, *args, rets.ctypes.data, max_returns,
                                                     lens.ctypes.data, status.ctypes.data,
                                                     counts.ctypes.data))
        self.func = None
        self._keep = keep
        lens = np.minimum(lens, max_returns)
        ints = ret_ints(rets)
        out = [[int(x) for x in ints[i][:lens[i]]] if status[i] == 0 else [] for i in range(self.n)]
        return out, status, counts

    # instance snapshots (WasmEdge_BatchSnapshotCreate / Restore)
    def snapshot(self, invocation=False):
        """Capture every instance's state as it stands between runs; returns a Snapshot.
        invocation=True (a resumable context after run() / resume()): the suspended invocation
        as well (WasmEdge_BatchSnapshotCreateSuspended) -- restore() then reinstates it and
        resume() continues it."""
        res = _Result(0)
        create = lib().WasmEdge_BatchSnapshotCreateSuspended if invocation else lib().WasmEdge_BatchSnapshotCreate
        h = create(self._h, ctypes.byref(res))
        if not h:
            raise WasmEdgeError(res.Code, lib().WasmEdge_BatchGetLastError(self._h).decode())
        return Snapshot(h)

    def restore(self, snap, src_of=None, timed=True):
        """Instance i restarts from the captured state of instance src_of[i] (None: its own);
        returns the restore kernels' time (timed=False: no host synchronisation, returns 0)."""
        if not isinstance(snap, Snapshot) or not snap._h:
            raise ValueError("a Snapshot that is not closed is needed")
        src = None
        if src_of is not None:
            src = np.ascontiguousarray(src_of, np.uint32)
            if src.shape != (self.n,):
                raise ValueError("src_of must have %d entries" % self.n)
        t = ctypes.c_double(0)
        self._check(lib().WasmEdge_BatchSnapshotRestore(self._h, snap._h,
                                                        src.ctypes.data if src is not None else None,
                                                        ctypes.byref(t) if timed else None))
        return t.value

    def restore_selected(self, snap, src_of, timed=True):
        """restore() that leaves some instances alone (WasmEdge_BatchSnapshotRestoreSelected):
        src_of[i] None or -1 keeps instance i as it is, any other entry restarts it from the
        captured state of that instance. Returns (kernel seconds, instances restored)."""
        if not isinstance(snap, Snapshot) or not snap._h:
            raise ValueError("a Snapshot that is not closed is needed")
        if src_of is None:
            raise ValueError("src_of is needed (restore() restores every instance from itself)")
        # an entry that does not fit 32 bits (or is negative and not -1) names no instance: it
        # goes to the library as one that is neither KEEP nor below n, and comes back as 0x04
        bad = KEEP - 1
        if isinstance(src_of, np.ndarray) and src_of.dtype.kind in "iu":   # (no per-entry loop)
            if src_of.dtype.kind == "u":
                wide = src_of.astype(np.uint64)
                wide = np.where(wide > KEEP, np.uint64(bad), wide)
            else:
                wide = src_of.astype(np.int64)
                wide = np.where(wide == -1, KEEP, np.where((wide < 0) | (wide > KEEP), bad, wide))
            src = np.ascontiguousarray(wide.astype(np.uint32))
        else:
            ints = [-1 if s is None else int(s) for s in src_of]
            src = np.array([KEEP if s == -1 else s if 0 <= s <= KEEP else bad for s in ints], np.uint32)
        if src.shape != (self.n,):
            raise ValueError("src_of must have %d entries" % self.n)
        t, r = ctypes.c_double(0), ctypes.c_uint32(0)
        self._check(lib().WasmEdge_BatchSnapshotRestoreSelected(self._h, snap._h, src.ctypes.data, ctypes.byref(r),
                                                                ctypes.byref(t) if timed else None))
        return t.value, int(r.value)

    def restore_tensor(self, snap, src_of, timed=True):
        """restore_selected() from a contiguous torch.int32 tensor [n] on the context's device
        (WasmEdge_BatchSnapshotRestoreSelectedDevice): -1 keeps the instance, the convention of
        func_of in set_calls_tensor; the map never crosses the host. Returns (kernel seconds,
        instances restored). The same note on torch initialising the device before the first
        BatchContext applies as for set_args_tensor."""
        torch = self._slot_tensor(src_of, None, "int32", "restore_tensor: src_of")
        if not isinstance(snap, Snapshot) or not snap._h:
            raise ValueError("a Snapshot that is not closed is needed")
        # the library does not know the stream that produced the tensor
        with torch.cuda.device(src_of.device):
            torch.cuda.current_stream().synchronize()
        t, r = ctypes.c_double(0), ctypes.c_uint32(0)
        self._check(lib().WasmEdge_BatchSnapshotRestoreSelectedDevice(self._h, snap._h, src_of.data_ptr(),
                                                                      ctypes.byref(r),
                                                                      ctypes.byref(t) if timed else None))
        return t.value, int(r.value)

    def total_costs(self):
        """Each instance's gas total (WasmEdge_BatchGetTotalCosts)."""
        c = np.zeros(self.n, np.uint64)
        self._check(lib().WasmEdge_BatchGetTotalCosts(self._h, c.ctypes.data))
        return c

    def memory_hash(self):
        h = np.zeros(self.n, np.uint64)
        self._check(lib().WasmEdge_BatchMemoryHash(self._h, h.ctypes.data))
        return h

    def memory(self, inst, off, length):
        buf = ctypes.create_string_buffer(length)
        self._check(lib().WasmEdge_BatchGetMemory(self._h, inst, off, buf, length))
        return buf.raw

    def memory_pages(self, inst):
        return lib().WasmEdge_BatchGetMemoryPages(self._h, inst)

    def code_size(self):
        return lib().WasmEdge_BatchGetCodeSize(self._h)

    def compiled_runs(self):
        """Straight-line runs compiled for the V-frame core (WasmEdge_BatchGetCompiledRuns)."""
        return lib().WasmEdge_BatchGetCompiledRuns(self._h)

    def memory_granule(self):
        """The interleave granule in use, bytes (WasmEdge_BatchGetMemoryGranule)."""
        return lib().WasmEdge_BatchGetMemoryGranule(self._h)

    def reserved_pages(self):
        """Pages of every instance in the directly addressed layout
        (WasmEdge_BatchGetReservedPages)."""
        return lib().WasmEdge_BatchGetReservedPages(self._h)

    def extra_memory_pages(self, mem):
        """Pages reserved per instance for memory `mem` >= 1 (WasmEdge_BatchGetExtraMemoryPages)."""
        return lib().WasmEdge_BatchGetExtraMemoryPages(self._h, mem)

    def engine(self):
        """The execution engine the context runs, e.g. "compiled-runs+simt/vgpr-frames"
        (WasmEdge_BatchGetEngine)."""
        return lib().WasmEdge_BatchGetEngine(self._h).decode()

    def interrupt(self):
        lib().WasmEdge_BatchInterrupt(self._h)

    def set_memory(self, inst, off, data):
        self._check(lib().WasmEdge_BatchSetMemory(self._h, inst, off, bytes(data), len(data)))

    # bulk transfer: every instance's linear memory in one call (WasmEdge_BatchWriteMemories /
    # ReadMemories and their Device variants). Instance i moves lens[i] (default: the row
    # length) bytes between row i and its memory at offset + offsets[i]; the returned status is
    # 0 or 0x88 per instance (out of bounds: that instance moved nothing).
    def _spans(self, offsets, lens):
        off = ln = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.uint32)
            if off.shape != (self.n,):
                raise ValueError("offsets must have %d entries" % self.n)
        if lens is not None:
            ln = np.ascontiguousarray(lens, np.uint32)
            if ln.shape != (self.n,):
                raise ValueError("lens must have %d entries" % self.n)
        return off, ln, (off.ctypes.data if off is not None else None,
                         ln.ctypes.data if ln is not None else None)

    def write_memories(self, data, offset=0, offsets=None, lens=None, length=None):
        """data: a uint8 array [n, stride], or a list of n bytes objects (padded to the
        longest; lens defaults to their lengths). length: the bytes of a row that count
        (default: the stride). Returns the status array."""
        if not isinstance(data, np.ndarray):
            items = [bytes(d) for d in data]
            if lens is None:
                lens = [len(d) for d in items]
            arr = np.zeros((len(items), max([len(d) for d in items] + [0])), np.uint8)
            for i, d in enumerate(items):
                arr[i, :len(d)] = np.frombuffer(d, np.uint8)
            data = arr
        data = np.ascontiguousarray(data, np.uint8)
        if data.ndim != 2 or data.shape[0] != self.n:
            raise ValueError("data must be [%d instances][stride], got shape %s" % (self.n, data.shape))
        off, ln, (po, pl) = self._spans(offsets, lens)
        status = np.zeros(self.n, np.uint8)
        length = data.shape[1] if length is None else length
        self._check(lib().WasmEdge_BatchWriteMemories(self._h, po, offset, pl, length,
                                                      data.ctypes.data if data.size else None,
                                                      data.shape[1], status.ctypes.data))
        return status

    def read_memories(self, length, offset=0, offsets=None, lens=None, out=None):
        """(uint8[n, length], status): row i holds instance i's bytes (zeros where it read
        nothing: past lens[i], or the whole row when its status is 0x88). out: a contiguous
        uint8 array [n, stride >= length] to read into instead; what an instance does not
        fill stays as it is."""
        if out is None:
            out = np.zeros((self.n, length), np.uint8)
        if out.dtype != np.uint8 or out.ndim != 2 or out.shape[0] != self.n or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array [%d instances][stride]" % self.n)
        off, ln, (po, pl) = self._spans(offsets, lens)
        status = np.zeros(self.n, np.uint8)
        self._check(lib().WasmEdge_BatchReadMemories(self._h, po, offset, pl, length,
                                                     out.ctypes.data if out.size else None, out.shape[1],
                                                     status.ctypes.data))
        return out, status

    def _tensor_io(self, fn, t, offset, offsets, lens):
        import torch
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] != self.n or not t.is_contiguous() \
                or not t.is_cuda:
            raise ValueError("a contiguous torch.uint8 tensor [%d, stride] on the device is needed" % self.n)
        off, ln, (po, pl) = self._spans(offsets, lens)
        status = np.zeros(self.n, np.uint8)
        # the library does not know the stream that produced (or will consume) the tensor
        with torch.cuda.device(t.device):
            torch.cuda.current_stream().synchronize()
        self._check(fn(self._h, po, offset, pl, t.shape[1], t.data_ptr() if t.numel() else None,
                       t.shape[1], status.ctypes.data))
        return status

    def write_memories_tensor(self, t, offset=0, offsets=None, lens=None):
        """write_memories from a contiguous torch.uint8 tensor [n, stride] on the context's
        device: the rows never cross the host. Returns the status array. A torch build that
        brings a HIP runtime of its own has to initialise the device (torch.cuda.init())
        before the process creates its first BatchContext: started second, that runtime
        finds no GPU."""
        return self._tensor_io(lib().WasmEdge_BatchWriteMemoriesDevice, t, offset, offsets, lens)

    def read_memories_tensor(self, t, offset=0, offsets=None, lens=None):
        """read_memories into such a tensor (bytes an instance does not fill stay as they
        are). Returns the status array."""
        return self._tensor_io(lib().WasmEdge_BatchReadMemoriesDevice, t, offset, offsets, lens)

    # device-resident spans (WasmEdge_BatchWriteMemoriesSpansDevice / ReadMemoriesSpansDevice):
    # the tensor variants above with every instance's own offset and length in int64 device
    # tensors -- the slot form of results_tensor, so a column view res[:, k] is passed as it is
    def _spans_tensor_io(self, fn, t, offsets, lens, offset, length, status):
        import sys
        torch = sys.modules.get("torch")
        if torch is None or not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 \
                or t.shape[0] != self.n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("a contiguous torch.uint8 tensor [%d, stride] on the device is needed" % self.n)
        for what, x in (("offsets", offsets), ("lens", lens)):
            if x is None:
                continue
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() != 1 or x.shape[0] != self.n \
                    or x.device != t.device or x.stride(0) <= 0:
                raise ValueError("%s: a one-dimensional torch.int64 tensor [%d] with a positive stride, on the "
                                 "device of the rows, is needed" % (what, self.n))
        if status is not None and (not isinstance(status, torch.Tensor) or status.dtype != torch.uint8
                                   or status.dim() != 1 or status.shape[0] != self.n
                                   or not status.is_contiguous() or status.device != t.device):
            raise ValueError("status: a contiguous torch.uint8 tensor [%d] on the device of the rows is needed" % self.n)
        length = t.shape[1] if length is None else int(length)
        if length < 0 or length > t.shape[1] or not 0 <= int(offset) < 1 << 32:
            raise ValueError("length must lie within a row and offset within 32 bits")
        # the library does not know the stream that produced (or will consume) the tensors
        with torch.cuda.device(t.device):
            torch.cuda.current_stream().synchronize()
        oob = ctypes.c_uint32(0)
        self._check(fn(self._h, offsets.data_ptr() if offsets is not None else None,
                       offsets.stride(0) if offsets is not None else 0, int(offset),
                       lens.data_ptr() if lens is not None else None, lens.stride(0) if lens is not None else 0,
                       length, t.data_ptr() if t.numel() else None, t.shape[1],
                       status.data_ptr() if status is not None else None, ctypes.addressof(oob)))
        return int(oob.value)

    def write_memories_spans_tensor(self, t, offsets=None, lens=None, offset=0, length=None, status=None):
        """write_memories_tensor with the spans on the device: instance i writes the first
        lens[i] (None: length; default: the row length) bytes of row i of t at offset +
        offsets[i] (None: 0). offsets / lens: one-dimensional torch.int64 tensors of n elements
        on t's device with any positive element stride -- a column view res[:, k] of a
        results_tensor output is accepted as it is; the low 32 bits of an element count.
        status: a contiguous torch.uint8 tensor [n] that receives 0 / 0x88 per instance, or
        None (no status bytes exist). Returns the number of instances out of bounds. Nothing
        per instance crosses the host. The same note on torch initialising the device before
        the first BatchContext applies as for write_memories_tensor."""
        return self._spans_tensor_io(lib().WasmEdge_BatchWriteMemoriesSpansDevice, t, offsets, lens, offset,
                                     length, status)

    def read_memories_spans_tensor(self, t, offsets=None, lens=None, offset=0, length=None, status=None):
        """read_memories_tensor with the spans on the device (write_memories_spans_tensor):
        bytes an instance does not fill stay as they are. Returns the number of instances out
        of bounds."""
        return self._spans_tensor_io(lib().WasmEdge_BatchReadMemoriesSpansDevice, t, offsets, lens, offset,
                                     length, status)

    def last_spans_tiled_waves(self):
        """Waves of the last spans transfer that took the tiled path
        (WasmEdge_BatchGetLastSpansTiledWaves). A report: results never depend on it."""
        return lib().WasmEdge_BatchGetLastSpansTiledWaves(self._h)

    # device-resident arguments and results (WasmEdge_BatchSetArgsDevice / ResultsDevice): rows
    # of 64-bit slots, one per value and two per v128 (low half first), as int64 tensors
    def _slot_tensor(self, t, width, dtype, what):
        """t is a contiguous tensor of torch dtype `dtype` on the device: [n, >= width] (width
        None: [n]). No torch import of its own: a caller with a tensor has imported it."""
        import sys
        torch = sys.modules.get("torch")
        shape = "[%d]" % self.n if width is None else "[%d, stride >= %d]" % (self.n, width)
        ok = torch is not None and isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) \
            and t.is_cuda and t.is_contiguous() and t.shape[0:1] == (self.n,) \
            and (t.dim() == 1 if width is None else t.dim() == 2 and t.shape[1] >= width)
        if not ok:
            raise ValueError("%s: a contiguous torch.%s tensor %s on the device is needed" % (what, dtype, shape))
        return torch

    def set_args_tensor(self, func, types, t):
        """set_args from a contiguous torch.int64 tensor [n, stride] on the context's device:
        row i holds instance i's arguments, one 64-bit slot per value (bit patterns for
        floats; the upper half of an i32 / f32 / funcref slot is ignored) and two per v128,
        stride >= slots_of(types); types: the parameters' value types, as make_values takes
        them. The values never cross the host. A torch build that brings a HIP runtime of its
        own has to initialise the device (torch.cuda.init()) before the process creates its
        first BatchContext: started second, that runtime finds no GPU."""
        types = [int(x) for x in types]
        width = slots_of(types)
        if width or t is not None:
            torch = self._slot_tensor(t, width, "int64", "set_args_tensor")
            # the library does not know the stream that produced the tensor
            with torch.cuda.device(t.device):
                torch.cuda.current_stream().synchronize()
        tarr = np.array(types, np.uint32)
        self._check(lib().WasmEdge_BatchSetArgsDevice(
            self._h, self._name(func), tarr.ctypes.data if len(types) else None, len(types),
            t.data_ptr() if t is not None and t.numel() else None, t.shape[1] if t is not None else 0))
        self.func = func
        self._keep = None

    def results_tensor(self, nret, out=None, status=None, counts=None):
        """results() into device tensors (WasmEdge_BatchResultsDevice): (out, status, counts).
        out: a contiguous torch.int64 tensor [n, stride], row i receiving instance i's first
        nret results in the slot form of set_args_tensor (zeroes when its status is not 0);
        slots of a row past them keep what they held. status: torch.uint8 [n]; counts:
        torch.int64 [n]. Each is allocated on the current torch device when None -- out as
        [n, nret], which fits unless a result is a v128 (two slots): then pass nret as the list
        of result types, or an out wide enough. The same note on torch initialising the device
        before the first BatchContext applies as for set_args_tensor."""
        width = None
        if not isinstance(nret, int):
            width = slots_of([int(x) for x in nret])
            nret = len(nret)
        if nret < 0:
            raise ValueError("results_tensor: nret must not be negative")
        given = [x for x in (out, status, counts) if x is not None]
        if out is not None:
            self._slot_tensor(out, width or 0, "int64", "results_tensor: out")
        if status is not None:
            self._slot_tensor(status, None, "uint8", "results_tensor: status")
        if counts is not None:
            self._slot_tensor(counts, None, "int64", "results_tensor: counts")
        import torch
        dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = torch.zeros((self.n, nret if width is None else width), dtype=torch.int64, device=dev)
        if status is None:
            status = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        if counts is None:
            counts = torch.zeros(self.n, dtype=torch.int64, device=dev)
        if out.device != dev or status.device != dev or counts.device != dev:
            raise ValueError("results_tensor: out, status and counts must be on one device")
        # the library does not know the stream that will consume (or last wrote) the tensors
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()
        self._check(lib().WasmEdge_BatchResultsDevice(
            self._h, out.data_ptr() if out.numel() else None, nret, out.shape[1],
            status.data_ptr(), counts.data_ptr()))
        return out, status, counts

    # device-resident per-instance calls (WasmEdge_BatchSetCallsDevice / CallsResultsDevice)
    def set_calls_tensor(self, funcs, func_of, rows, types=None):
        """set_calls from device tensors: funcs = the export names; func_of: a contiguous
        torch.int32 tensor [n] on the context's device, instance i's index into funcs or -1 (no
        call); rows: a contiguous torch.int64 tensor [n, stride], row i holding the arguments
        of funcs[func_of[i]] in the slot form of set_args_tensor from slot 0 on, or None when
        nothing takes parameters; types: None (the module's signatures are taken as they are)
        or one list of value types per name, checked against the module (a difference gives
        the instances naming that function 0x83). Neither tensor crosses the host. The same
        note on torch initialising the device before the first BatchContext applies as for
        set_args_tensor."""
        names, arr, tptrs, tlens, keep = call_names(funcs, types)
        torch = self._slot_tensor(func_of, None, "int32", "set_calls_tensor: func_of")
        if rows is not None:
            self._slot_tensor(rows, 0, "int64", "set_calls_tensor: rows")
            if rows.device != func_of.device:
                raise ValueError("set_calls_tensor: func_of and rows must be on one device")
        # the library does not know the stream that produced the tensors
        with torch.cuda.device(func_of.device):
            torch.cuda.current_stream().synchronize()
        self._check(lib().WasmEdge_BatchSetCallsDevice(
            self._h, arr, len(names), tptrs, tlens, func_of.data_ptr(),
            rows.data_ptr() if rows is not None and rows.numel() else None,
            rows.shape[1] if rows is not None else 0))
        self.func = None
        self._keep = None

    def calls_results_tensor(self, width, out=None, lens=None, status=None, counts=None):
        """results() / return_lens() after set_calls or set_calls_tensor into device tensors
        (WasmEdge_BatchCallsResultsDevice): (out, lens, status, counts). out: a contiguous
        torch.int64 tensor [n, stride >= width]; row i receives exactly `width` slots, its
        function's result slots first and then zeroes (all zeroes when its status is not 0 or
        it sat the run out); width must cover the widest result row of the staged functions.
        lens: torch.int32 [n] (each function's result count); status: torch.uint8 [n]; counts:
        torch.int64 [n]. Each is allocated on the current torch device when None, out as
        [n, width]."""
        if not isinstance(width, int) or isinstance(width, bool) or width < 0:
            raise ValueError("calls_results_tensor: width must be a non-negative int")
        given = [x for x in (out, lens, status, counts) if x is not None]
        if out is not None:
            self._slot_tensor(out, width, "int64", "calls_results_tensor: out")
        if lens is not None:
            self._slot_tensor(lens, None, "int32", "calls_results_tensor: lens")
        if status is not None:
            self._slot_tensor(status, None, "uint8", "calls_results_tensor: status")
        if counts is not None:
            self._slot_tensor(counts, None, "int64", "calls_results_tensor: counts")
        import torch
        dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = torch.zeros((self.n, width), dtype=torch.int64, device=dev)
        if lens is None:
            lens = torch.zeros(self.n, dtype=torch.int32, device=dev)
        if status is None:
            status = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        if counts is None:
            counts = torch.zeros(self.n, dtype=torch.int64, device=dev)
        if any(x.device != dev for x in (out, lens, status, counts)):
            raise ValueError("calls_results_tensor: out, lens, status and counts must be on one device")
        # the library does not know the stream that will consume (or last wrote) the tensors
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()
        self._check(lib().WasmEdge_BatchCallsResultsDevice(
            self._h, out.data_ptr() if out.numel() else None, width, out.shape[1],
            lens.data_ptr(), status.data_ptr(), counts.data_ptr()))
        return out, lens, status, counts

    # exported tables / globals of one instance (WasmEdge_TableInstance*/GlobalInstance*);
    # inst=None writes every instance
    def table_size(self, name, inst):
        n = ctypes.c_uint32(0)
        self._check(lib().WasmEdge_BatchTableGetSize(self._h, self._name(name), inst, ctypes.byref(n)))
        return n.value

    def table_get(self, name, inst, off):
        v = _Value()
        self._check(lib().WasmEdge_BatchTableGetData(self._h, self._name(name), inst, ctypes.byref(v), off))
        return v.int(), v.type

    def table_set(self, name, inst, off, value, vtype):
        inst = ALL_INSTANCES if inst is None else inst
        self._check(lib().WasmEdge_BatchTableSetData(self._h, self._name(name), inst,
                                                     _Value.make(value, vtype), off))

    def global_get(self, name, inst):
        v = _Value()
        self._check(lib().WasmEdge_BatchGlobalGetValue(self._h, self._name(name), inst, ctypes.byref(v)))
        return v.int(), v.type

    def global_set(self, name, inst, value, vtype):
        inst = ALL_INSTANCES if inst is None else inst
        self._check(lib().WasmEdge_BatchGlobalSetValue(self._h, self._name(name), inst,
                                                       _Value.make(value, vtype)))

    def add_host_function(self, module, name, fn, nparams, nresults, cost=0):
        """Bind `fn(mem: HostMemory, args: list[int]) -> (code, results: list[int])` to
        the import module.name (WasmEdge_BatchAddHostFunction; with a gas `cost`,
        WasmEdge_BatchAddHostFunctionWithCost). Values are raw bits (uint128 as python
        ints); code 0 = success, else the ErrCode ending the instance (0x01 Terminated)."""
        def tramp(_data, memcxt, params, returns):
            pv = np.ctypeslib.as_array((ctypes.c_uint8 * (32 * max(nparams, 1))).from_address(params)) \
                if nparams else None
            args = []
            if nparams:
                vals = pv.view(VALUE_DTYPE)
                args = [int(vals["lo"][k]) | (int(vals["hi"][k]) << 64) for k in range(nparams)]
            try:
                code, res = fn(HostMemory(memcxt), args)
            except WasmEdgeError as e:
                return e.code
            if code == 0 and nresults:
                rv = np.ctypeslib.as_array((ctypes.c_uint8 * (32 * nresults)).from_address(returns)).view(VALUE_DTYPE)
                for k in range(nresults):
                    v = int(res[k]) & ((1 << 128) - 1)
                    rv["lo"][k] = v & 0xFFFFFFFFFFFFFFFF
                    rv["hi"][k] = v >> 64
            return code
        cb = HOST_FUNC(tramp)
        self._hosts = getattr(self, "_hosts", []) + [cb]   # keep the trampoline alive
        self._check(lib().WasmEdge_BatchAddHostFunctionWithCost(self._h, self._name(module),
                                                                self._name(name), cb, None, cost))


    # built-in WASI subset (WasmEdge_BatchInitWASIWithPreopens): args/envs shared by every
    # instance, preopened directories as fds 3, 4, ...
    def init_wasi(self, args=(), envs=(), preopens=()):
        a, e, p = _cstrs(args), _cstrs(envs), _cstrs(preopens)
        self._check(lib().WasmEdge_BatchInitWASIWithPreopens(self._h, a, len(args), e, len(envs),
                                                             p, len(preopens)))

    def wasi_deterministic(self, seed, clock_ns):
        """Reproducible fd numbers / random_get / clocks (WasmEdge_BatchWASISetDeterministic)."""
        self._check(lib().WasmEdge_BatchWASISetDeterministic(self._h, seed, clock_ns))

    def set_instance_args(self, inst, args):
        """Instance `inst`'s own command line (WasmEdge_BatchWASISetInstanceArgs)."""
        self._check(lib().WasmEdge_BatchWASISetInstanceArgs(self._h, inst, _cstrs(args), len(args)))

    def wasi_exit_code(self, inst):
        return lib().WasmEdge_BatchWASIGetExitCode(self._h, inst)

    def wasi_output(self, inst, fd=1):
        n = lib().WasmEdge_BatchWASIGetOutput(self._h, inst, fd, None, 0)
        buf = ctypes.create_string_buffer(max(n, 1))
        lib().WasmEdge_BatchWASIGetOutput(self._h, inst, fd, buf, n)
        return buf.raw[:n]


class Snapshot:
    """The captured state of a BatchContext's instances (WasmEdge_BatchSnapshot), held on the
    device until close(). It belongs to the context it was taken from and may be closed
    before or after it."""

    def __init__(self, handle):
        self._h = handle

    @property
    def nbytes(self):
        """Device bytes the snapshot holds."""
        return int(lib().WasmEdge_BatchSnapshotGetBytes(self._h)) if self._h else 0

    @property
    def suspended(self):
        """Suspended instances the snapshot holds (0 unless taken with invocation=True)."""
        return int(lib().WasmEdge_BatchSnapshotGetSuspendedCount(self._h)) if self._h else 0

    def close(self):
        if getattr(self, "_h", None):
            lib().WasmEdge_BatchSnapshotDelete(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _cstrs(v):
    v = list(v)
    return (ctypes.c_char_p * max(len(v), 1))(*[x.encode() for x in v])


def ret_ints(rets):
    """Return values (VALUE_DTYPE array) as python ints (uint128)."""
    lo = rets["lo"].astype(object)
    hi = rets["hi"].astype(object)
    return lo + hi * (1 << 64)
