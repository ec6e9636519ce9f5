"""Resumable runs (WasmEdge_BatchConfigure::Resumable, WasmEdge_BatchResume,
WasmEdge_BatchGetSuspendedCount): an instance that ends a run with Interrupted (0x07) is
suspended on the device and continues where it stopped. The reference has no counterpart,
so the yardstick is slice invariance: a run cut into slices of s instructions ends with the
returns, statuses, counts, memory hashes and gas totals of the oracle's uninterrupted run
(compare(exact=True)), and after every slice a suspended instance has status 0x07 and a
count >= the limit while a finished instance's row already equals its final row."""
import ctypes
import functools
import os
import subprocess
import threading

import pytest

import oracle_py as O
import calls_cases as K
from helpers import ROOT, compare
from wasmedge_amd.wat import assemble

I32, I64 = 0x7F, 0x7E
SUSPENDED = 0x07

FIB = assemble(r"""
(module
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2))))))))
""")

# a short loop: 1 + i % 23 trips, counts of a few hundred at most
SHORT = assemble(r"""
(module
  (func (export "tri") (param $n i32) (result i32) (local $i i32) (local $s i32)
    (loop $l
      (local.set $s (i32.add (local.get $s) (i32.mul (local.get $i) (local.get $i))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br_if $l (i32.lt_u (local.get $i) (local.get $n))))
    (local.get $s)))
""")

# sum(n) by plain recursion: depth n takes ~2n call-stack cells, so n >= 3000 leaves the LDS
# slots and passes the 4096-cell reservation (tests/test_deepstack.py): the stack doubles
SUM = assemble(r"""
(module
  (func $sum (export "sum") (param $n i32) (result i32)
    (if (result i32) (i32.eqz (local.get $n))
      (then (i32.const 0))
      (else (i32.add (local.get $n) (call $sum (i32.sub (local.get $n) (i32.const 1))))))))
""")

# i32 and i64 stores at per-instance addresses in the last page, memory.grow once mid-way
MEM = assemble(r"""
(module
  (memory 1 4)
  (func (export "fill") (param $n i32) (param $base i32) (result i32) (local $i i32) (local $a i32)
    (loop $l
      (local.set $a (i32.add (i32.add (local.get $base) (i32.shl (local.get $i) (i32.const 4)))
                             (i32.shl (i32.sub (memory.size) (i32.const 1)) (i32.const 16))))
      (i32.store (local.get $a) (i32.mul (i32.add (local.get $i) (i32.const 1)) (i32.const 40503)))
      (i64.store offset=8 (local.get $a) (i64.mul (i64.extend_i32_u (local.get $a)) (i64.const 0x100000001)))
      (if (i32.eq (local.get $i) (i32.shr_u (local.get $n) (i32.const 1)))
        (then (drop (memory.grow (i32.const 1)))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br_if $l (i32.lt_u (local.get $i) (local.get $n))))
    (memory.size)))
""")

# a host call every iteration; the trip count depends on the lane
HOSTLOOP = assemble(r"""
(module
  (import "env" "add_i64" (func $add (param i64 i64) (result i64)))
  (func (export "acc") (param $n i32) (result i64) (local $i i32) (local $s i64)
    (block $done
      (loop $l
        (br_if $done (i32.ge_u (local.get $i) (local.get $n)))
        (local.set $s (call $add (local.get $s) (i64.extend_i32_u (i32.mul (local.get $i) (i32.const 7)))))
        (local.set $i (i32.add (local.get $i) (i32.const 1)))
        (br $l)))
    (local.get $s)))
""")

# waits for a non-zero word at address 0, returns it
WAIT = assemble(r"""
(module
  (memory 1)
  (func (export "wait") (result i32)
    (loop $l (br_if $l (i32.eqz (i32.load (i32.const 0)))))
    (i32.load (i32.const 0))))
""")

# tests/test_metering.py test_gpu_interrupt's counting loop
COUNT = assemble("(module (func (export \"count\") (param i32) (result i32) (local i32)"
                 " (loop $l (local.set 1 (i32.add (local.get 1) (i32.const 1)))"
                 " (br_if $l (i32.lt_u (local.get 1) (local.get 0)))) (local.get 1)))")


# ----------------------------------------------------------------------------- CPU
def test_null_context_without_a_device(built):
    """The product library loads without a device; the new entry points take NULL."""
    from wasmedge_amd import batch
    L = batch.lib()
    assert L.WasmEdge_BatchResume(None, 0, None).Code == 0x04
    assert L.WasmEdge_BatchResume(None, 1000, ctypes.byref(ctypes.c_double(0))).Code == 0x04
    assert L.WasmEdge_BatchGetSuspendedCount(None) == 0


def test_conf_mirror_matches_header(tmp_path):
    """batch._Conf against the C compiler's layout of WasmEdge_BatchConfigure."""
    from wasmedge_amd import batch
    src = tmp_path / "conf.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wasmedge_batch.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu\\n", sizeof(WasmEdge_BatchConfigure),\n'
                   "         offsetof(WasmEdge_BatchConfigure, Resumable));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "conf"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert ctypes.sizeof(batch._Conf) == size
    assert batch._Conf.Resumable.offset == off


# ----------------------------------------------------------------------------- GPU
# the engine matrix of tests/test_calls.py (restated: that file is not imported)
ENGINES = {
    "simt": {},                                   # V frames, compiled runs, SIMT scheduling
    "trip": {"WB_TRIP": "1"},                     # V frames, trip mode
    "nosimt": {"WB_SIMT": "0"},                   # V frames, compiled runs without SIMT
    "nojit": {"WB_JIT": "0"},                     # V frames, threaded core handlers only
    "lds": {"WB_VFRAME": "0"},                    # LDS frames, threaded core
    "step": {"WB_THREADED": "0"},                 # the compiled C++ step only
    "hbm": {"WB_HBMFRAME": "1"},                  # frames in HBM (compiled step)
}


@functools.lru_cache(maxsize=None)
def _oracle(wasm, func, args):
    return O.Module(wasm).run(func, list(args))


def _ref(wasm, func, rows):
    return [_oracle(wasm, func, tuple(r)) for r in rows]


def _cap(ref, s):
    """Slices a run cut every s instructions can take: every resume below an instance's
    final count retires at least one instruction of it, so ceil(max count / s), + 2."""
    return -(-max(r[2] for r in ref) // s) + 2


def _ctx(wasm, n, **kw):
    from wasmedge_amd import batch
    kw.setdefault("device", 0)
    if kw.get("devices") is not None:
        kw.pop("device")
    kw.setdefault("resumable", True)
    return batch.BatchContext(wasm, n, **kw)


def _rows(ctx, nret):
    from wasmedge_amd import batch
    rets, st, cnt = ctx.results(nret)
    ints = batch.ret_ints(rets)
    return [(int(st[i]), int(cnt[i]), [int(x) for x in ints[i]]) for i in range(ctx.n)]


def _slices(ctx, s, cap, nret, each=None):
    """After run() under max_steps = s: resume(k * s), k = 2, 3, ... until nothing is
    suspended, at most `cap` slices (s = 0: resume(0), no count bound to check). After
    every slice: a suspended instance has 0x07, zeroed returns and a count >= the limit; a
    finished instance's row never changes again; suspended() is their number. each(k, prev,
    rows) sees consecutive slices. Returns (slices, final rows)."""
    done, prev, k = {}, None, 1
    while True:
        rows = _rows(ctx, nret)
        nsusp = 0
        for i, r in enumerate(rows):
            if r[0] == SUSPENDED:
                nsusp += 1
                assert i not in done, (k, i)
                assert r[1] >= k * s and not any(r[2]), (k, i, r)
            else:
                assert done.setdefault(i, r) == r, (k, i, done[i], r)
        assert ctx.suspended() == nsusp, (k, nsusp)
        if each:
            each(k, prev, rows)
        if nsusp == 0:
            return k, rows
        k += 1
        assert k <= cap, "still suspended after %d slices" % cap
        ctx.resume(k * s)
        prev = rows


def _final(ctx, ref, rows, rtypes):
    got = [r[2][:len(rtypes)] if r[0] == 0 else [] for r in rows]
    st, cnt = [r[0] for r in rows], [r[1] for r in rows]
    assert compare(ref, got, st, cnt, ctx.memory_hash(), rtypes, exact=True) == []


def _start(ctx, func, rows, ptypes):
    from wasmedge_amd import batch
    ctx.set_args(func, batch.make_values(rows, ptypes))
    ctx.run()


def _invariant(wasm, func, rows, ptypes, rtypes, s, **kw):
    ref = _ref(wasm, func, rows)
    ctx = _ctx(wasm, len(rows), max_steps=s, **kw)
    try:
        _start(ctx, func, rows, ptypes)
        k, out = _slices(ctx, s, _cap(ref, s), len(rtypes))
        _final(ctx, ref, out, rtypes)
        return k
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("s", [1000, 12347])
def test_gpu_resume_every_engine(built, monkeypatch, engine, n, s):
    """Divergent recursion fib(10 + i % 7) cut every s instructions, through every engine."""
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    k = _invariant(FIB, "fib", [[10 + i % 7] for i in range(n)], [I32], [I32], s)
    assert k > 1, "nothing was ever suspended"


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["simt", "nojit"])
def test_gpu_resume_single_step(built, monkeypatch, engine):
    """The limit raised by 1 per resume: an instance below the new limit retires at least one
    instruction, one already at it (a dispatch retires several) is suspended again as it is."""
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    n = 65
    rows = [[1 + i % 23] for i in range(n)]
    ref = _ref(SHORT, "tri", rows)
    assert 100 < max(r[2] for r in ref) < 1000

    def each(k, prev, cur):
        for i in range(n):
            if prev is not None and prev[i][0] == SUSPENDED:
                if prev[i][1] < k:
                    assert cur[i][1] > prev[i][1], (k, i, prev[i], cur[i])
                else:
                    assert cur[i] == prev[i], (k, i, prev[i], cur[i])

    ctx = _ctx(SHORT, n, max_steps=1)
    try:
        _start(ctx, "tri", rows, [I32])
        _, out = _slices(ctx, 1, _cap(ref, 1), 1, each)
        _final(ctx, ref, out, [I32])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_stack_growth(built, n):
    """sum(3000 + i): the call stack leaves the LDS slots and doubles mid-invocation
    (CallStackCells 0) while other lanes of the wave are suspended; their frames and stack
    slots survive the relayout. s: a prime near a tenth of the count."""
    rows = [[3000 + i] for i in range(n)]
    ref = _ref(SUM, "sum", rows)
    s = 3607
    assert 8 * s < ref[0][2] < 12 * s, ref[0][2]
    assert _invariant(SUM, "sum", rows, [I32], [I32], s) >= 9


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_memory(built, n):
    """Stores and a memory.grow across slice boundaries: hashes and sizes as uninterrupted."""
    rows = [[40 + i % 9, 64 * (i % 100)] for i in range(n)]
    ref = _ref(MEM, "fill", rows)
    assert all(r[0] == 0 and r[1] == [2] for r in ref)
    ctx = _ctx(MEM, n, max_steps=101)
    try:
        _start(ctx, "fill", rows, [I32, I32])
        k, out = _slices(ctx, 101, _cap(ref, 101), 1)
        assert k > 3
        _final(ctx, ref, out, [I32])
        assert [ctx.memory_pages(i) for i in range(n)] == [2] * n
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_host_imports_in_the_wave(built, n):
    """Within one launch some lanes park at the import while others of their wave are
    suspended; the host function is called as often per instance as uninterrupted."""
    from hostfuncs import add_i64
    rows = [[3 + (i * 5) % 17] for i in range(n)]
    ref = _ref(HOSTLOOP, "acc", rows)
    calls = {}

    def counted(mem, a):
        calls[mem.instance] = calls.get(mem.instance, 0) + 1
        return add_i64(mem, a)

    def run(s, resumable):
        calls.clear()
        ctx = _ctx(HOSTLOOP, n, max_steps=s, resumable=resumable)
        try:
            ctx.add_host_function("env", "add_i64", counted, 2, 1)
            _start(ctx, "acc", rows, [I32])
            k, out = _slices(ctx, s, _cap(ref, s) if s else 1, 1)
            _final(ctx, ref, out, [I64])
            return k, dict(calls)
        finally:
            ctx.close()

    _, whole = run(0, False)
    assert whole == {i: rows[i][0] for i in range(n)}
    k, sliced = run(37, True)
    assert k > 3 and sliced == whole


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_metered(built, n):
    """CostLimit between fib(13)'s and fib(14)'s cost: the larger arguments end with
    CostLimitExceeded (0x03) mid-way, stay so and are never resumed; gas totals as
    uninterrupted."""
    rows = [[10 + i % 7] for i in range(n)]
    limit = (_oracle(FIB, "fib", (13,))[2] + _oracle(FIB, "fib", (14,))[2]) // 2
    m = O.Module(FIB)
    insts = [O.Instance(m, cost_limit=limit) for _ in range(n)]
    ref = [x.invoke("fib", r) for x, r in zip(insts, rows)]
    assert {r[0] for r in ref} == {0, 0x03}
    s = 1000
    ctx = _ctx(FIB, n, max_steps=s, cost_limit=limit)
    try:
        _start(ctx, "fib", rows, [I32])
        k, out = _slices(ctx, s, _cap(ref, s), 1)
        assert k > 3
        _final(ctx, ref, out, [I32])
        assert [int(c) for c in ctx.total_costs()] == [x.cost_sum() for x in insts]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_call_vector(built, n):
    """tests/calls_cases.py's mixed vector: NO_CALL, unknown-name and mismatch rows stay
    0 / 0x05 / 0x83 with count 0 through every resume, the rest are slice-invariant, and
    return_lens does not change."""
    from hostfuncs import add_i64
    vec = K.mixed_vector(n)
    ref = K.oracle_rows(vec)
    s = 1000
    ctx = _ctx(K.CALLS, n, max_steps=s)
    try:
        ctx.add_host_function("env", "add_i64", add_i64, 2, 1)
        ctx.set_calls(vec.funcs, vec.func_of, vec.rows)
        ctx.run()
        lens = [int(x) for x in ctx.return_lens()]
        assert lens == [len(K.RTYPES[vec.name(i)]) if vec.expect[i] is None else 0 for i in range(n)]

        def each(k, prev, cur):
            for i in range(n):
                if vec.expect[i] is not None:
                    assert cur[i] == (vec.expect[i], 0, [0, 0]), (k, i, cur[i])
            assert [int(x) for x in ctx.return_lens()] == lens, k

        k, out = _slices(ctx, s, _cap(ref, s), 2, each)
        assert k > 3
        got = [r[2][:lens[i]] if r[0] == 0 else [] for i, r in enumerate(out)]
        assert compare(ref, got, [r[0] for r in out], [r[1] for r in out], ctx.memory_hash(), None,
                       exact=True) == []
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_resume_feeds_a_waiting_instance(built, n):
    """Instances spin on a word of their memory; the host writes it between slices."""
    import numpy as np
    from wasmedge_amd import batch
    word = [0x1000 + i for i in range(n)]
    data = np.array(word, "<u4").view(np.uint8).reshape(n, 4)
    odds = n // 2
    ctx = _ctx(WAIT, n, max_steps=5000)
    try:
        ctx.set_args("wait", np.zeros((n, 0), batch.VALUE_DTYPE))
        ctx.run()
        assert ctx.suspended() == n and all(r[0] == SUSPENDED for r in _rows(ctx, 1))
        assert not ctx.write_memories(data, lens=[4 * (1 - i % 2) for i in range(n)]).any()
        ctx.resume(10000)
        rows = _rows(ctx, 1)
        for i, r in enumerate(rows):
            if i % 2:
                assert r[0] == SUSPENDED and r[1] >= 10000 and r[2] == [0], (i, r)
            else:
                assert r[0] == 0 and r[2] == [word[i]], (i, r)
        assert ctx.suspended() == odds
        assert not ctx.write_memories(data, lens=[4 * (i % 2) for i in range(n)]).any()
        ctx.resume(20000)
        assert ctx.suspended() == 0
        after = _rows(ctx, 1)
        assert [r[0] for r in after] == [0] * n and [r[2][0] for r in after] == word
        assert all(after[i] == rows[i] for i in range(0, n, 2))   # the evens' rows stayed
    finally:
        ctx.close()


def _count_to_the_end(ctx, n, trips):
    """resume(0) until done, at most 200 slices; every instance ends with `trips`."""
    k = 1
    while ctx.suspended():
        k += 1
        assert k <= 200
        ctx.resume(0)
    rows = _rows(ctx, 1)
    assert [r[0] for r in rows] == [0] * n and [r[2][0] for r in rows] == [trips] * n
    return k, [r[1] for r in rows]


# a counting loop that lasts a few tenths of a second: a 0.05 s slice is far shorter
TRIPS = 3_000_000


@pytest.mark.gpu
def test_gpu_resume_time_limit(built):
    """TimeLimitSeconds = 0.05 cuts the loop into slices (the clock starts anew with each
    call); the final count equals the uninterrupted run's."""
    from wasmedge_amd import batch
    n = 65
    vals = batch.make_values([[TRIPS]] * n, [I32])
    whole = batch.BatchContext(COUNT, n, device=0, time_limit=60.0)
    try:
        _, st, want = whole.execute("count", vals, 1)
        assert not st.any()
    finally:
        whole.close()
    ctx = _ctx(COUNT, n, time_limit=0.05)
    try:
        ctx.set_args("count", vals)
        ctx.run()
        assert ctx.suspended() == n, "the loop is too short for the limit to cut it"
        k, cnt = _count_to_the_end(ctx, n, TRIPS)
        assert cnt == [int(c) for c in want], k
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_resume_after_interrupt(built):
    """One run stopped by WasmEdge_BatchInterrupt from a timer, then resume(0) to the end;
    the request is cleared when the resume starts."""
    from wasmedge_amd import batch
    n = 65
    ctx = _ctx(COUNT, n, time_limit=60.0)
    try:
        ctx.set_args("count", batch.make_values([[TRIPS]] * n, [I32]))
        t = threading.Timer(0.05, ctx.interrupt)
        t.start()
        ctx.run()
        t.join()
        assert ctx.suspended() == n, "the loop ended before the interrupt"
        k, _ = _count_to_the_end(ctx, n, TRIPS)
        assert k == 2
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_resume_lifecycle(built):
    """What ends a suspended invocation (0x04 afterwards), what does not, and a snapshot
    taken while suspended."""
    from wasmedge_amd import batch
    n = 65
    rows = [[10 + i % 7] for i in range(n)]
    ref = _ref(FIB, "fib", rows)
    vals = batch.make_values(rows, [I32])

    def refused(ctx):
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.resume(0)
        assert e.value.code == 0x04

    plain = _ctx(FIB, n, max_steps=1000, resumable=False)
    try:
        plain.set_args("fib", vals)
        plain.run()
        assert plain.suspended() == 0
        refused(plain)
    finally:
        plain.close()

    ctx = _ctx(FIB, n, max_steps=1000)
    try:
        refused(ctx)                       # before any run
        ctx.set_args("fib", vals)
        ctx.run()
        assert ctx.suspended() == n
        snap = ctx.snapshot()              # legal while suspended; frames are not captured
        assert ctx.suspended() == n
        ctx.reset()
        assert ctx.suspended() == 0
        refused(ctx)
        ctx.set_args("fib", vals)
        ctx.run()
        ctx.set_args("fib", vals)
        refused(ctx)
        ctx.run()
        ctx.set_calls(["fib"], [0] * n, [[(r[0], I32)] for r in rows])
        refused(ctx)
        # a run ends the invocation before it and begins its own: part of the way, then a
        # new run, which starts from the top and is the one a resume continues
        ctx.run()
        ctx.resume(5000)
        assert 0 < ctx.suspended() < n
        ctx.run()
        assert ctx.suspended() == n
        k, out = _slices(ctx, 1000, _cap(ref, 1000), 1)
        _final(ctx, ref, out, [I32])
        ctx.restore(snap)
        refused(ctx)
        # the restored snapshot run afresh: as a fresh run, nothing of the old frames is used
        ctx.set_args("fib", vals)
        ctx.run()
        k, out = _slices(ctx, 1000, _cap(ref, 1000), 1)
        _final(ctx, ref, out, [I32])
        # nothing suspended: success, no launch, the results as they were
        assert ctx.resume(0) == 0.0 and ctx.suspended() == 0
        assert _rows(ctx, 1) == out
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("partition", [0, 1])
def test_gpu_resume_shards(built, partition):
    """Devices = [0, 0]: BatchResume goes to every shard, GetSuspendedCount sums them; equal
    to the single-device run."""
    n, s = 130, 1000
    rows = [[10 + i % 7] for i in range(n)]
    ref = _ref(FIB, "fib", rows)
    one = _ctx(FIB, n, max_steps=s)
    two = _ctx(FIB, n, max_steps=s, devices=[0, 0], partition=partition)
    try:
        outs = []
        for ctx in (one, two):
            _start(ctx, "fib", rows, [I32])
            assert ctx.suspended() == n
            k, out = _slices(ctx, s, _cap(ref, s), 1)
            _final(ctx, ref, out, [I32])
            outs.append((k, out))
        assert outs[0] == outs[1]
    finally:
        one.close()
        two.close()
