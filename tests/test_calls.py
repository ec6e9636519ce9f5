"""Per-instance calls (WasmEdge_BatchSetCalls / ExecuteCalls / GetReturnLens): each instance
of a batch runs its own export, as N independent WasmEdge_VMExecute calls would
(lib/vm/vm.cpp:287-308 resolves each name, lib/executor/executor.cpp:88-100 checks each
signature). Expected values: the oracle running every instance's export on its own
(oracle_py.Module.run, Instance.invoke); instances that do not run (NO_CALL, an unknown
name 0x05, a signature mismatch 0x83) have count 0, no returns and the memory of a fresh
instance. Everything is compared bit for bit (compare(exact=True))."""
import ctypes
import functools

import pytest

import oracle_py as O
import calls_cases as K
from helpers import compare, emu_lib
from wasmedge_amd.wat import assemble

I32, I64 = K.I32, K.I64


@functools.lru_cache(maxsize=None)
def _mixed(n, k=len(K.NAMES)):
    vec = K.mixed_vector(n, k)
    return vec, K.oracle_rows(vec)


# ----------------------------------------------------------------------------- CPU
def test_oracle_vector_covers_the_cases():
    """The vector's own outcomes: traps (0x84) among the br_table loop's lanes, a NaN
    payload through the multi-value export, every kind of lane that does not run."""
    vec, ref = _mixed(130)
    codes = {r[0] for r in ref}
    assert {0, 0x84, K.NOT_FOUND, K.SIG_MISMATCH} <= codes, codes
    mv = [r for i, r in enumerate(ref) if vec.expect[i] is None and vec.name(i) == "mv"]
    assert any(r[1][1] == K.NAN_PAYLOAD ^ (1 << 63) for r in mv)
    assert [vec.expect[i] for i in K.NO_CALL_LANES] == [0, 0, 0, 0]
    assert sorted(vec.expect[i] for i in (K.UNKNOWN_LANE, K.WRONG_LEN_LANE, K.WRONG_TYPE_LANE)) == \
        [K.NOT_FOUND, K.SIG_MISMATCH, K.SIG_MISMATCH]


def test_emulator_calls_match_oracle(built):
    """N = 130, function i % k, with the non-running lanes in the same vector: status,
    count, returns and memory hash per instance against the oracle."""
    from hostfuncs import emu_host
    vec, ref = _mixed(130)
    rets, st, cnt, h, raw = K.emu_run_calls(K.CALLS, vec, host=emu_host(K.IMPORTS))
    assert compare(ref, rets, st, cnt, h, None, exact=True) == []
    for i in range(vec.n):
        if vec.expect[i] is not None:
            assert int(st[i]) == vec.expect[i] and int(cnt[i]) == 0, i
            assert int(h[i]) == K.fresh_hash(), i
            assert not raw[i].any(), i   # returns zeroed


def test_emulator_func_of_out_of_range(built):
    vec = K.mixed_vector(8)
    vec.func_of[2] = len(vec.funcs)
    with pytest.raises(RuntimeError, match="0x4"):
        K.emu_run_calls(K.CALLS, vec)
    assert b"names no function" in emu_lib().wb_emu_last_error()


# ----------------------------------------------------------------------------- GPU
# the engine matrix of tests/test_workloads.py (restated: that file is not imported)
ENGINES = {
    "simt": {},                                   # V frames, compiled runs, SIMT scheduling
    "trip": {"WB_TRIP": "1"},                     # V frames, trip mode
    "nosimt": {"WB_SIMT": "0"},                   # V frames, compiled runs without SIMT
    "nojit": {"WB_JIT": "0"},                     # V frames, threaded core handlers only
    "lds": {"WB_VFRAME": "0"},                    # LDS frames, threaded core
    "step": {"WB_THREADED": "0"},                 # the compiled C++ step only
    "hbm": {"WB_HBMFRAME": "1"},                  # frames in HBM (compiled step)
}


def _ctx(wasm, n, **kw):
    from hostfuncs import add_i64
    from wasmedge_amd import batch
    kw.setdefault("device", 0)
    if kw.get("devices") is not None:
        kw.pop("device")
    ctx = batch.BatchContext(wasm, n, **kw)
    ctx.add_host_function("env", "add_i64", add_i64, 2, 1)
    return ctx


def _run(ctx, vec):
    rets, st, cnt = ctx.execute_calls(vec.funcs, vec.func_of, vec.rows)
    return rets, st, cnt, ctx.memory_hash()


def _check_idle(vec, st, cnt):
    for i in range(vec.n):
        if vec.expect[i] is not None:
            assert int(st[i]) == vec.expect[i] and int(cnt[i]) == 0, i


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("n", [8, 65, 130])
def test_gpu_calls_every_engine(built, monkeypatch, engine, n):
    """The mixed vector (idle lanes at 0, 63, 64, 129 and among running ones) through every
    engine: no engine may run an idle lane, read its params or write its results."""
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    vec, ref = _mixed(n)
    ctx = _ctx(K.CALLS, n)
    try:
        rets, st, cnt, h = _run(ctx, vec)
        assert compare(ref, rets, st, cnt, h, None, exact=True) == [], (engine, ctx.engine())
        _check_idle(vec, st, cnt)
        lens = [int(x) for x in ctx.return_lens()]
        assert lens == [len(K.RTYPES[vec.name(i)]) if vec.expect[i] is None else 0 for i in range(n)]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_result_rows(built):
    """BatchResults after SetCalls: ReturnLen is the row stride, each row carries its
    function's result types, the values past them and idle rows are zeroed."""
    from wasmedge_amd import batch
    vec, ref = _mixed(65)
    ctx = _ctx(K.CALLS, 65)
    try:
        ctx.set_calls(vec.funcs, vec.func_of, vec.rows)
        ctx.run()
        rets, st, cnt = ctx.results(3)
        ints = batch.ret_ints(rets)
        for i in range(65):
            rt = K.RTYPES[vec.name(i)] if vec.expect[i] is None else []
            assert [int(t) for t in rets["type"][i][:len(rt)]] == rt, i
            want = list(ref[i][1]) if ref[i][0] == 0 else [0] * len(rt)
            assert [int(x) for x in ints[i]] == want + [0] * (3 - len(rt)), i
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_whole_wave_layouts(built):
    """N = 192: wave 0 all one function, wave 1 entirely NO_CALL, wave 2 mixed."""
    base = K.mixed_vector(192)
    func_of, rows, expect = list(base.func_of), list(base.rows), list(base.expect)
    for i in range(64):
        func_of[i], expect[i] = 0, None
        rows[i] = [(K.args_of("fib", i)[0], I32)]
    for i in range(64, 128):
        func_of[i], expect[i] = None, 0
    vec = K.Vector(base.funcs, func_of, rows, expect)
    ref = K.oracle_rows(vec)
    ctx = _ctx(K.CALLS, 192)
    try:
        rets, st, cnt, h = _run(ctx, vec)
        assert compare(ref, rets, st, cnt, h, None, exact=True) == []
        _check_idle(vec, st, cnt)
    finally:
        ctx.close()


def _seq_rounds(n):
    """poke-or-NO_CALL, then peek by everyone, on the same instances."""
    poke = K.Vector(["poke"], [None if i % 3 == 1 else 0 for i in range(n)],
                    [[((i * 4) % 4096, I32), (0xC0DE0000 + i, I32)] for i in range(n)],
                    [0 if i % 3 == 1 else None for i in range(n)])
    peek = K.Vector(["peek"], [0] * n, [[((i * 4) % 4096, I32)] for i in range(n)], [None] * n)
    return poke, peek


def _seq_oracle(n, rounds):
    m = K.module()
    insts = [O.Instance(m) for _ in range(n)]
    out = []
    for vec in rounds:
        if isinstance(vec, tuple):   # (name, rows): a uniform run
            out.append([x.invoke(vec[0], r) for x, r in zip(insts, vec[1])])
            continue
        rows = []
        for i, x in enumerate(insts):
            if vec.expect[i] is not None:   # sits the run out: its memory as it was
                rows.append((vec.expect[i], [], 0, x.invoke("tick", [])[3]))
            else:
                rows.append(x.invoke(vec.name(i), [v for v, _ in vec.rows[i]]))
        out.append(rows)
    return out


@pytest.mark.gpu
def test_gpu_calls_state_persists(built):
    """Run 1: every instance pokes its own address or sits out; run 2: every instance
    peeks, no Reset between; then a uniform SetArgs run on the same context; then Reset and
    the same again."""
    from wasmedge_amd import batch
    n = 130
    poke, peek = _seq_rounds(n)
    uni = ("fib", [[(i * 5) % 13] for i in range(n)])
    ref = _seq_oracle(n, [poke, peek, uni])
    ctx = _ctx(K.CALLS, n)
    try:
        for rep in range(2):
            for r, vec in enumerate((poke, peek)):
                rets, st, cnt, h = _run(ctx, vec)
                assert compare(ref[r], rets, st, cnt, h, None, exact=True) == [], (rep, r)
            rets, st, cnt = ctx.execute("fib", batch.make_values(uni[1], [I32]), 1)
            ints = batch.ret_ints(rets)
            got = [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(n)]
            assert compare(ref[2], got, st, cnt, ctx.memory_hash(), [I32], exact=True) == [], rep
            ctx.reset()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_host_import_in_mixed_wave(built):
    """Lanes calling the export that calls env.add_i64 park while the others of their wave
    finish; the oracle binds the same host module."""
    n = 130
    names = ["hostadd", "fib", "walk"]
    func_of = [None if i in K.NO_CALL_LANES else i % 3 for i in range(n)]
    rows = [[(v, t) for v, t in zip(K.args_of(names[i % 3], i), K.PTYPES[names[i % 3]])] for i in range(n)]
    vec = K.Vector(names, func_of, rows, [0 if f is None else None for f in func_of])
    ref = K.oracle_rows(vec)
    assert any(r[0] == 0x84 for r in ref)
    ctx = _ctx(K.CALLS, n)
    try:
        rets, st, cnt, h = _run(ctx, vec)
        assert compare(ref, rets, st, cnt, h, None, exact=True) == []
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_metered(built):
    """CostLimit (unit table) low enough that some lanes end with CostLimitExceeded (0x03):
    statuses, counts and gas totals against oracle instances with the same limit; a lane
    that does not run keeps the gas total of instantiation."""
    n, limit = 130, 60
    vec = K.mixed_vector(n, 6)   # (without the host import's export)
    m = K.module()
    insts = [O.Instance(m, cost_limit=limit) for _ in range(n)]
    ref = []
    for i, x in enumerate(insts):
        if vec.expect[i] is not None:
            ref.append((vec.expect[i], [], 0, K.fresh_hash()))
        else:
            ref.append(x.invoke(vec.name(i), [v for v, _ in vec.rows[i]]))
    codes = {r[0] for r in ref}
    assert 0x03 in codes and 0 in codes, codes
    ctx = _ctx(K.CALLS, n, cost_limit=limit)
    try:
        rets, st, cnt, h = _run(ctx, vec)
        assert compare(ref, rets, st, cnt, h, None, exact=True) == []
        _check_idle(vec, st, cnt)
        assert [int(c) for c in ctx.total_costs()] == [x.cost_sum() for x in insts]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("partition", [0, 1])
def test_gpu_calls_shards(built, partition):
    """Devices = [0, 0]: FuncOf / Params / ParamLens sliced by the placement, the outputs
    gathered in instance order -- equal to the single-device run."""
    n = 130
    vec, ref = _mixed(n)
    one = _ctx(K.CALLS, n)
    two = _ctx(K.CALLS, n, devices=[0, 0], partition=partition)
    try:
        a, b = _run(one, vec), _run(two, vec)
        assert compare(ref, *b, None, exact=True) == []
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert [int(v) for v in x] == [int(v) for v in y]
        assert [int(v) for v in one.return_lens()] == [int(v) for v in two.return_lens()]
    finally:
        one.close()
        two.close()


@pytest.mark.gpu
def test_gpu_calls_layout_trial(built):
    """MemoryGranule 0 on a module the lowering marks divergent_mem (the quicksort, with a
    second trivial export): four Reset + Run rounds alternating two call vectors. A
    measurement on one vector never settles the trial begun on the other; every round is
    bit-exact and the granule in use is a legal one."""
    import wasmedge_amd.workloads as W
    src = W.qsort_wat()
    wasm = assemble(src[:src.rindex(")")] +
                    '  (func (export "inc") (param $x i32) (result i32) (i32.add (local.get $x) (i32.const 1))))')
    n = 130
    m = O.Module(wasm)

    def vector(flip):
        fo = [(i + flip) % 2 for i in range(n)]
        rows = [[(i, I32), ((i * 37) % 300, I32)] if f == 0 else [(i, I32)] for i, f in enumerate(fo)]
        return K.Vector(["sort", "inc"], fo, rows, [None] * n)

    vecs = [vector(0), vector(1)]
    refs = [[m.run(v.name(i), [x for x, _ in v.rows[i]]) for i in range(n)] for v in vecs]
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm, n, device=0, memory_granule=0)
    try:
        for rnd in range(4):
            ctx.reset()
            rets, st, cnt, h = _run(ctx, vecs[rnd % 2])
            assert compare(refs[rnd % 2], rets, st, cnt, h, None, exact=True) == [], rnd
            assert ctx.memory_granule() in (4, 128), rnd   # (the trial's two layouts)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_persistent_waves(built):
    """More waves than the device holds at once (2,048 at the V-frame kernel's two per
    SIMD): persistent waves take batch waves from a counter, in the longest-first order
    learned from the last launch of an equal vector. The same vector twice (the second
    launch uses the learned order), then another vector (which must not): results,
    statuses and counts of every instance each time."""
    import numpy as np
    wasm = assemble(r"""
(module
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2)))))))
  (func (export "inc") (param $x i32) (result i32) (i32.add (local.get $x) (i32.const 1))))
""")
    n = 2048 * 64 + 3 * 64 + 5
    m = O.Module(wasm)
    fibs = {a: m.run("fib", [a]) for a in range(3, 10)}
    inc_cnt = m.run("inc", [0])[2]
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm, n, device=0)
    try:
        for shift in (0, 0, 1):
            kind = [(i + shift) % 3 for i in range(n)]   # 0 fib, 1 inc, 2 NO_CALL
            rows = [[(i % 7 + 3, I32)] if k == 0 else [(i, I32)] if k == 1 else [] for i, k in enumerate(kind)]
            ctx.set_calls(["fib", "inc"], [None if k == 2 else k for k in kind], rows)
            ctx.run()
            rets, st, cnt = ctx.results(1)
            want = np.array([fibs[i % 7 + 3][1][0] if k == 0 else (i + 1) & 0xFFFFFFFF if k == 1 else 0
                             for i, k in enumerate(kind)], np.uint64)
            wcnt = np.array([fibs[i % 7 + 3][2] if k == 0 else inc_cnt if k == 1 else 0
                             for i, k in enumerate(kind)], np.uint64)
            assert not st.any(), shift
            assert np.array_equal(rets["lo"][:, 0], want), shift
            assert np.array_equal(cnt, wcnt), shift
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_calls_call_level_errors(built):
    """A FuncOf entry that is neither NO_CALL nor < NumFuncs fails the call with 0x04 and
    leaves the previous staging as it was; so does a NULL context."""
    from wasmedge_amd import batch
    vec, ref = _mixed(65)
    ctx = _ctx(K.CALLS, 65)
    try:
        ctx.set_calls(vec.funcs, vec.func_of, vec.rows)
        bad = list(vec.func_of)
        bad[9] = len(vec.funcs)
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.set_calls(vec.funcs, bad, vec.rows)
        assert e.value.code == 0x04
        ctx.run()
        lens = ctx.return_lens()
        rets, st, cnt = ctx.results(2)
        ints = batch.ret_ints(rets)
        got = [[int(x) for x in ints[i][:lens[i]]] if st[i] == 0 else [] for i in range(65)]
        assert compare(ref, got, st, cnt, ctx.memory_hash(), None, exact=True) == []
    finally:
        ctx.close()
    L = batch.lib()
    fo = (ctypes.c_uint32 * 1)(batch.NO_CALL)
    assert L.WasmEdge_BatchSetCalls(None, None, 0, fo, None, 0, None).Code == 0x04
    assert L.WasmEdge_BatchExecuteCalls(None, None, 0, fo, None, 0, None, None, 0, None, None, None).Code == 0x04
    assert L.WasmEdge_BatchGetReturnLens(None, fo).Code == 0x04


@pytest.mark.gpu
def test_gpu_calls_host_import_export_refused(built):
    """An exported host import among the called names fails the run as a uniform
    BatchRun on it does."""
    from wasmedge_amd import batch
    wasm = assemble(r"""
(module
  (import "env" "add_i64" (func $add (param i64 i64) (result i64)))
  (export "add" (func $add))
  (func (export "one") (result i32) (i32.const 1)))
""")
    ctx = _ctx(wasm, 8)
    try:
        ctx.set_calls(["one", "add"], [0] * 7 + [1], [[]] * 7 + [[(1, I64), (2, I64)]])
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.run()
        assert e.value.code == 0x02
        rets, st, cnt = ctx.execute_calls(["one", "add"], [0] * 7 + [None], [[]] * 8)
        assert rets == [[1]] * 7 + [[]] and [int(s) for s in st] == [0] * 8
    finally:
        ctx.close()
