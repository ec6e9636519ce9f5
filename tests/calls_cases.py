"""Per-instance calls (WasmEdge_BatchSetCalls): the test module, the call vectors and their
oracle references, shared by tests/test_calls.py. The oracle runs every instance's export on
its own (oracle_py.Module.run / Instance.invoke), which is what N independent
WasmEdge_VMExecute calls are."""
import ctypes
import functools

import numpy as np

import oracle_py as O
from helpers import CELLS, emu_lib, from_cells, to_cells
from wasmedge_amd.wat import assemble

I32, I64, F32, F64, V128 = 0x7F, 0x7E, 0x7D, 0x7C, 0x7B
NOT_FOUND, SIG_MISMATCH = 0x05, 0x83

# Exports of different signatures on one memory: a recursive fib, a br_table loop that
# divides by a parameter (0x84 where it is 0 and the dividing arm is reached), poke / peek on
# memory, a multi-value (f64, v128) -> (v128, f64) whose f64 result keeps a NaN payload,
# a () -> i64, and one that calls the host import env.add_i64.
CALLS = assemble(r"""
(module
  (import "env" "add_i64" (func $add (param i64 i64) (result i64)))
  (memory 1)
  (data (i32.const 0) "\01\02\03\04\05\06\07\08\09\0a\0b\0c\0d\0e\0f\10\11\12\13\14\15\16\17\18")
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2)))))))
  (func (export "walk") (param $x i32) (param $d i32) (result i32)
    (local $i i32) (local $acc i32)
    (block $done
      (loop $l
        (br_if $done (i32.ge_u (local.get $i) (i32.const 12)))
        (block $b2
          (block $b1
            (block $b0
              (br_table $b0 $b1 $b2 (i32.rem_u (i32.add (local.get $x) (local.get $i)) (i32.const 3))))
            (local.set $acc (i32.add (local.get $acc) (i32.div_u (local.get $x) (local.get $d))))
            (local.set $i (i32.add (local.get $i) (i32.const 1)))
            (br $l))
          (local.set $acc (i32.xor (local.get $acc) (local.get $i)))
          (local.set $i (i32.add (local.get $i) (i32.const 2)))
          (br $l))
        (local.set $acc (i32.add (i32.mul (local.get $acc) (i32.const 3)) (i32.const 1)))
        (local.set $i (i32.add (local.get $i) (i32.const 1)))
        (br $l)))
    (local.get $acc))
  (func (export "poke") (param $a i32) (param $v i32)
    (i32.store (local.get $a) (local.get $v)))
  (func (export "peek") (param $a i32) (result i32)
    (i32.load (local.get $a)))
  (func (export "mv") (param $f f64) (param $v v128) (result v128 f64)
    (i64x2.add (local.get $v) (i64x2.splat (i64.reinterpret_f64 (local.get $f))))
    (f64.neg (local.get $f)))
  (func (export "tick") (result i64)
    (i64.add (i64.load (i32.const 8)) (i64.const 0x1122334455667788)))
  (func (export "hostadd") (param $x i64) (result i64)
    (call $add (local.get $x) (i64.load (i32.const 0)))))
""")

NAMES = ["fib", "walk", "poke", "peek", "mv", "tick", "hostadd"]
PTYPES = {"fib": [I32], "walk": [I32, I32], "poke": [I32, I32], "peek": [I32], "mv": [F64, V128],
          "tick": [], "hostadd": [I64]}
RTYPES = {"fib": [I32], "walk": [I32], "poke": [], "peek": [I32], "mv": [V128, F64], "tick": [I64],
          "hostadd": [I64]}
IMPORTS = ["add_i64"]   # (import order, for hostfuncs.emu_host)
NAN_PAYLOAD = 0x7FF80000DEADBEEF


def args_of(name, i):
    return {"fib": [(i * 7) % 15],
            "walk": [(i * 13 + 1) & 0xFFFFFFFF, i % 4],
            "poke": [(i * 4) % 4096, (i * 2654435761 + 1) & 0xFFFFFFFF],
            "peek": [(i * 4) % 4096],
            "mv": [NAN_PAYLOAD if i % 3 == 0 else 0x4009000000000000 + i,
                   ((i * 0x0123456789ABCDEF) & ((1 << 64) - 1)) | ((i + 1) << 64)],
            "tick": [],
            "hostadd": [i * 1000003]}[name]


class Vector:
    """A call vector: funcs (names), func_of (index or None) and rows ((value, type) pairs)
    per instance, and expect[i] = None where the instance runs, else the status it sits the
    run out with (0 NO_CALL, 0x05, 0x83)."""

    def __init__(self, funcs, func_of, rows, expect):
        self.funcs, self.func_of, self.rows, self.expect = funcs, func_of, rows, expect
        self.n = len(func_of)

    def name(self, i):
        return None if self.func_of[i] is None else self.funcs[self.func_of[i]]


NO_CALL_LANES = (0, 63, 64, 129)
UNKNOWN_LANE, WRONG_LEN_LANE, WRONG_TYPE_LANE = 5, 6, 7


def mixed_vector(n, k=len(NAMES)):
    """Instance i calls NAMES[i % k]; NO_CALL at lanes 0, 63, 64 and 129, one unknown name,
    one wrong ParamLens and one wrong value type (the lanes above)."""
    funcs = NAMES[:k] + ["nosuch"]
    func_of, rows, expect = [], [], []
    for i in range(n):
        name = NAMES[i % k]
        f, row, e = i % k, [(v, t) for v, t in zip(args_of(name, i), PTYPES[name])], None
        if i in NO_CALL_LANES:
            f, e = None, 0
        elif i == UNKNOWN_LANE:
            f, e = k, NOT_FOUND
        elif i == WRONG_LEN_LANE:
            row, e = row + [(1, I32)], SIG_MISMATCH
        elif i == WRONG_TYPE_LANE:
            f, row, e = 0, [(3, I64)], SIG_MISMATCH   # fib(i64)
        func_of.append(f)
        rows.append(row)
        expect.append(e)
    return Vector(funcs, func_of, rows, expect)


@functools.lru_cache(maxsize=None)
def module():
    return O.Module(CALLS)


@functools.lru_cache(maxsize=None)
def fresh_hash():
    """Memory hash of a freshly instantiated instance (tick reads memory only)."""
    return module().run("tick", [])[3]


def oracle_rows(vec):
    """(code, values, count, memhash) per instance, each on a fresh instance."""
    out = []
    for i in range(vec.n):
        if vec.expect[i] is not None:
            out.append((vec.expect[i], [], 0, fresh_hash()))
        else:
            out.append(module().run(vec.name(i), [v for v, _ in vec.rows[i]]))
    return out


def emu_run_calls(wasm, vec, host=None, cost_limit=0, max_pages=0):
    """wb_emu_execute_calls on the vector: (rets, st, cnt, h) as helpers.emu_run."""
    E = emu_lib()
    E.wb_emu_set_tail_call(0)
    E.wb_emu_set_multi_memory(0)
    E.wb_emu_set_host(host)
    E.wb_emu_set_cost_limit(cost_limit)
    E.wb_emu_set_cost_table(None, 0)
    n = vec.n
    pstride = max([len(r) for r in vec.rows] + [1])
    pcstride = max([sum(CELLS[t] for _, t in r) for r in vec.rows] + [1])
    rcstride = max([sum(CELLS[t] for t in rt) for rt in RTYPES.values()] + [1])
    params = np.zeros((n, pcstride), np.uint32)
    ptypes = np.zeros((n, pstride), np.uint8)
    plens = np.zeros(n, np.uint32)
    for i, r in enumerate(vec.rows):
        cells = to_cells([v for v, _ in r], [t for _, t in r])
        params[i, :len(cells)] = cells
        ptypes[i, :len(r)] = [t for _, t in r]
        plens[i] = len(r)
    names = [f.encode() for f in vec.funcs]
    arr = (ctypes.c_char_p * max(len(names), 1))(*names)
    fo = np.array([0xFFFFFFFF if f is None else f for f in vec.func_of], np.uint32)
    res = np.zeros((n, rcstride), np.uint32)
    rlens = np.zeros(n, np.uint32)
    st = np.zeros(n, np.uint8)
    cnt = np.zeros(n, np.uint64)
    h = np.zeros(n, np.uint64)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    E.wb_emu_execute_calls.argtypes = [ctypes.c_char_p, u32, ctypes.POINTER(ctypes.c_char_p), u32, vp,
                                       u32, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp,
                                       u32, u32, ctypes.c_uint64]
    e = E.wb_emu_execute_calls(wasm, len(wasm), arr, len(names), fo.ctypes.data, n, params.ctypes.data,
                               pcstride, ptypes.ctypes.data, pstride, plens.ctypes.data, res.ctypes.data,
                               rcstride, rlens.ctypes.data, st.ctypes.data, cnt.ctypes.data, h.ctypes.data,
                               max_pages, 0, 0)
    if e:
        raise RuntimeError("emu error 0x%x: %s" % (e, E.wb_emu_last_error().decode()))
    rets = []
    for i in range(n):
        name = vec.name(i)
        rt = RTYPES.get(name, []) if vec.expect[i] is None else []
        assert int(rlens[i]) == len(rt), (i, int(rlens[i]), rt)
        rets.append(from_cells(res[i], rt) if st[i] == 0 else [])
    return rets, st, cnt, h, res
