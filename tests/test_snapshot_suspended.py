"""Snapshots of suspended runs (WasmEdge_BatchSnapshotCreateSuspended,
WasmEdge_BatchSnapshotGetSuspendedCount; Python: BatchContext.snapshot(invocation=True),
Snapshot.suspended): a snapshot taken between the slices of a resumable run holds the
suspended invocation as well, and WasmEdge_BatchSnapshotRestore reinstates it, so that
BatchResume continues instance i exactly as instance SrcOf[i] would have from the capture.

The yardstick is the oracle's uninterrupted run, as in tests/test_resume.py (whose modules,
engine matrix and helpers are used here): after a rewind every instance ends with its own
oracle row, after a fork with its source's -- status, returns, count and memory hash bit for
bit (helpers.compare(exact=True)) -- however the run was cut and wherever it was captured.
N = 65 and 130: a partial last wave, and two waves plus a partial one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import test_resume as TR
from helpers import ROOT, compare
from test_resume import COUNT, FIB, HOSTLOOP, I32, I64, MEM, SUM, SUSPENDED, WAIT   # noqa: F401
from wasmedge_amd.wat import assemble

# fib beside an export that traps and one with two results (i64, i32): three result-row shapes
MIXED = assemble(r"""
(module
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2)))))))
  (func (export "boom") (param $n i32) (result i32)
    (unreachable))
  (func (export "pair") (param $n i32) (result i64 i32)
    (i64.mul (i64.extend_i32_u (local.get $n)) (i64.const 0x100000001))
    (i32.add (local.get $n) (i32.const 1))))
""")


# ----------------------------------------------------------------------------- CPU
def test_null_arguments_without_a_device(built):
    from wasmedge_amd import batch
    L = batch.lib()
    res = batch._Result(0x55)
    assert L.WasmEdge_BatchSnapshotCreateSuspended(None, ctypes.byref(res)) is None
    assert res.Code == 0x04
    assert L.WasmEdge_BatchSnapshotCreateSuspended(None, None) is None
    assert L.WasmEdge_BatchSnapshotGetSuspendedCount(None) == 0


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "susp_abi.c"
    src.write_text('#include "wasmedge_batch.h"\n'
                   "WasmEdge_BatchSnapshot *take(WasmEdge_BatchContext *c, WasmEdge_Result *r) {\n"
                   "  return WasmEdge_BatchSnapshotCreateSuspended(c, r); }\n"
                   "uint32_t held(const WasmEdge_BatchSnapshot *s) { return WasmEdge_BatchSnapshotGetSuspendedCount(s); }\n")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "susp_abi.o")])


STACK_MAIN = r"""
#include <stdio.h>
#include "snapshot_plan.h"
// stdin: n gs_lds gs_depth has_src, then nwaves*64 LS_RPC, nwaves*64 LS_GSP, then n sources;
// stdout: per wave "rows offset", the total, per wave "class rows", the depth needed
int main() {
  unsigned n, lds, depth, has;
  if (scanf("%u %u %u %u", &n, &lds, &depth, &has) != 4) return 2;
  const unsigned nw = (n + 63) / 64;
  std::vector<uint32_t> rpc(nw * 64), gsp(nw * 64), src(n), rows, wave;
  std::vector<uint64_t> off;
  for (auto &x : rpc) if (scanf("%u", &x) != 1) return 2;
  for (auto &x : gsp) if (scanf("%u", &x) != 1) return 2;
  for (unsigned i = 0; i < n && has; i++) if (scanf("%u", &src[i]) != 1) return 2;
  const uint64_t total = wbs::pack_stack(rpc.data(), gsp.data(), n, nw, lds, depth, &rows, &off);
  for (unsigned w = 0; w < nw; w++) printf("%u %llu\n", rows[w], (unsigned long long)off[w]);
  printf("%llu\n", (unsigned long long)total);
  wbs::RestorePlan P;
  wbs::plan_restore(has ? src.data() : nullptr, n, nw, rows.data(), true, &P);
  const uint32_t need = wbs::plan_stack(has ? P.src.data() : nullptr, nw, rows.data(), &wave);
  for (unsigned w = 0; w < nw; w++) printf("%u %u\n", wave[2 * w], wave[2 * w + 1]);
  printf("%u\n", need);
  return 0;
}
"""


@pytest.fixture(scope="module")
def stack_prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("stackplan")
    (d / "main.cpp").write_text(STACK_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "wasmedge_amd", "csrc"), str(d / "main.cpp"), "-o", str(d / "plan")])
    return str(d / "plan")


NOT_PARKED = 0xFFFFFFFF
PLAN_N, PLAN_LDS, PLAN_DEPTH = 300, 24, 1000   # five waves, the last partial; a depth that is no multiple of 64


def _plan_lanes():
    """LS_RPC / LS_GSP of 5 waves. Wave 0: nothing parked (deep but stale LS_GSP). Wave 1: the
    deepest parked lane exactly at gs_lds, others below it. Wave 2: one parked lane one cell
    past gs_lds, a deeper lane that is not parked. Wave 3: a parked lane at the allocated
    depth (gs_lds + gs_depth cells) and one claiming more. Wave 4 (44 instances): depths 65
    and 129 rows; its lanes past n are parked and deep, and do not count."""
    rpc, gsp = [NOT_PARKED] * 320, [0] * 320
    for l in range(64):
        gsp[l] = 500 + l
    for l in range(64):
        rpc[64 + l], gsp[64 + l] = 10 + l, PLAN_LDS if l == 7 else l % PLAN_LDS
    rpc[128 + 3], gsp[128 + 3] = 5, PLAN_LDS + 1
    gsp[128 + 9] = 900
    rpc[192 + 63], gsp[192 + 63] = 1, PLAN_LDS + PLAN_DEPTH
    rpc[192 + 1], gsp[192 + 1] = 1, PLAN_LDS + PLAN_DEPTH + 77
    rpc[256], gsp[256] = 2, PLAN_LDS + 65
    rpc[256 + 43], gsp[256 + 43] = 2, PLAN_LDS + 129
    for l in range(44, 64):
        rpc[256 + l], gsp[256 + l] = 3, 4000
    return rpc, gsp


def _model_rows(rpc, gsp):
    rows = []
    for w in range(5):
        deepest = max([max(0, gsp[i] - PLAN_LDS) for i in range(w * 64, min(w * 64 + 64, PLAN_N))
                       if rpc[i] != NOT_PARKED] + [0])
        rows.append(min(-(-deepest // 64) * 64, PLAN_DEPTH))
    return rows


PLAN_MAPS = {
    "identity": None,
    "broadcast": [PLAN_N - 1] * PLAN_N,
    "reverse": [PLAN_N - 1 - i for i in range(PLAN_N)],
    "within": [(i & ~63) | ((i + 5) % (64 if i < 256 else 44)) for i in range(PLAN_N)],
    "random": [int(x) for x in np.random.RandomState(5).randint(0, PLAN_N, PLAN_N)],
    "shallow": [64 + i % 128 for i in range(PLAN_N)],   # sources of waves 1 and 2 only
}


@pytest.mark.parametrize("name", sorted(PLAN_MAPS))
def test_stack_plan_against_model(stack_prog, name):
    """The call-stack rows a capture holds per wave (S_w), their offsets, and for a restore
    every destination wave's class and rows and the depth the stack needs."""
    rpc, gsp = _plan_lanes()
    src = PLAN_MAPS[name]
    text = "%d %d %d %d\n%s\n%s\n%s\n" % (PLAN_N, PLAN_LDS, PLAN_DEPTH, 0 if src is None else 1,
                                       " ".join(map(str, rpc)), " ".join(map(str, gsp)),
                                       " ".join(map(str, src or [])))
    out = subprocess.run([stack_prog], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = _model_rows(rpc, gsp)
    assert rows == [0, 0, 64, PLAN_DEPTH, 192]
    off = 0
    for w in range(5):
        assert out[w].split() == [str(rows[w]), str(off)], (w, out[w])
        off += rows[w] * 64
    assert int(out[5]) == off
    need = 0
    for w in range(5):
        # a lane past n follows lane 0 of its wave into that lane's source wave
        lanes = [i if src is None else src[i] if i < PLAN_N else (src[i & ~63] & ~63) | (i & 63)
                 for i in range(w * 64, w * 64 + 64)]
        cls = 0 if lanes == list(range(w * 64, w * 64 + 64)) else 1 if len({s >> 6 for s in lanes}) == 1 else 2
        most = max(rows[s >> 6] for s in lanes)
        assert out[6 + w].split() == [str(cls), str(most)], (w, out[6 + w])
        need = max(need, most)
    assert int(out[11]) == need
    assert need == {"identity": 1000, "broadcast": 192, "reverse": 1000, "within": 1000, "shallow": 64}.get(name, need)


# ----------------------------------------------------------------------------- GPU
def _go(ctx, s, k, cap, nret, each=None):
    """From the state after slice k (a capture point or a restore of one): resume((k + 1) * s),
    ... until nothing is suspended, with test_resume._slices' checks after every slice.
    Returns (slices, final rows)."""
    done = {}
    while True:
        rows = TR._rows(ctx, nret)
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
            each(k, rows)
        if nsusp == 0:
            return k, rows
        k += 1
        assert k <= cap, "still suspended after %d slices" % cap
        ctx.resume(k * s)


def _to(ctx, s, k0, k1):
    for k in range(k0 + 1, k1 + 1):
        ctx.resume(k * s)
    return k1


def _mapped(ref, src):
    return [ref[s] for s in src]


def _nsusp(rows, src=None):
    return sum(1 for i in range(len(rows)) if rows[src[i] if src else i][0] == SUSPENDED)


FIB_S, FIB_K = 1000, 4   # fib(10), fib(11) end below 4000 instructions, fib(12) .. fib(16) above


def _fib_rows(n):
    return [[10 + i % 7] for i in range(n)]


def _fib_state(n, **kw):
    """fib(10 + i % 7) under slices of 1000: run, then one resume to 4000."""
    rows = _fib_rows(n)
    ref = TR._ref(FIB, "fib", rows)
    assert max(r[2] for r in ref if r[1][0] <= 89) < FIB_K * FIB_S < min(r[2] for r in ref if r[1][0] > 89)
    ctx = TR._ctx(FIB, n, max_steps=FIB_S, **kw)
    TR._start(ctx, "fib", rows, [I32])
    ctx.resume(FIB_K * FIB_S)
    return ctx, ref


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(TR.ENGINES))
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_rewind_every_engine(built, monkeypatch, engine, n):
    """Capture with finished and suspended instances in the batch, finish, restore, finish
    again from the same k, twice: the same rows, the oracle's."""
    for k, v in TR.ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    ctx, ref = _fib_state(n)
    try:
        rec, nsusp = TR._rows(ctx, 1), ctx.suspended()
        assert 0 < nsusp < n and nsusp == _nsusp(rec)
        snap = ctx.snapshot(invocation=True)
        assert snap.suspended == nsusp and ctx.suspended() == nsusp and TR._rows(ctx, 1) == rec
        cap = TR._cap(ref, FIB_S)
        ka, a = _go(ctx, FIB_S, FIB_K, cap, 1)
        TR._final(ctx, ref, a, [I32])
        hashes = [int(h) for h in ctx.memory_hash()]
        for _ in range(2):
            ctx.restore(snap)
            assert ctx.suspended() == nsusp and snap.suspended == nsusp
            assert TR._rows(ctx, 1) == rec
            kb, b = _go(ctx, FIB_S, FIB_K, cap, 1)
            assert (kb, b) == (ka, a)
            TR._final(ctx, ref, b, [I32])
            assert [int(h) for h in ctx.memory_hash()] == hashes
        snap.close()
    finally:
        ctx.close()


def _fork_maps(n, rec):
    first = next(i for i, r in enumerate(rec) if r[0] == SUSPENDED)
    last = max(i for i, r in enumerate(rec) if r[0] == SUSPENDED)
    return {"broadcast_first": [first] * n, "broadcast_last": [last] * n,
            "reverse": [n - 1 - i for i in range(n)],
            "random": [int(x) for x in np.random.RandomState(n).randint(0, n, n)]}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_fork(built, n):
    """Broadcast of one suspended instance, reversal (across waves at 130) and a fixed random
    map: instance i ends with the oracle row of instance SrcOf[i], count included."""
    ctx, ref = _fib_state(n)
    try:
        rec = TR._rows(ctx, 1)
        snap = ctx.snapshot(invocation=True)
        cap = TR._cap(ref, FIB_S)
        for name, src in _fork_maps(n, rec).items():
            if name == "reverse":
                ctx.reset()   # (a fork is legal whatever the context did since)
            ctx.restore(snap, src)
            assert ctx.suspended() == _nsusp(rec, src), name
            assert TR._rows(ctx, 1) == _mapped(rec, src), name
            if name.startswith("broadcast"):
                assert ctx.suspended() == n
            _, out = _go(ctx, FIB_S, FIB_K, cap, 1)
            TR._final(ctx, _mapped(ref, src), out, [I32])
        # a run needs its arguments staged again after a fork
        from wasmedge_amd import batch
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.run()
        assert e.value.code == 0x04
        TR._start(ctx, "fib", _fib_rows(n), [I32])
        _, out = TR._slices(ctx, FIB_S, cap, 1)
        TR._final(ctx, ref, out, [I32])
        snap.close()
    finally:
        ctx.close()


def _mixed_vector(n):
    """i % 5 == 0: no call; 1: boom (0x89); 3: pair (two results, ends in the first slice);
    else fib(11 + i % 6)."""
    funcs = ["fib", "boom", "pair"]
    func_of = [None if i % 5 == 0 else 1 if i % 5 == 1 else 2 if i % 5 == 3 else 0 for i in range(n)]
    rows = [[(11 + i % 6 if func_of[i] == 0 else i, I32)] for i in range(n)]
    fresh = TR._oracle(MIXED, "pair", (0,))[3]   # (no memory: every hash is the fresh one)
    ref = [(0, [], 0, fresh) if f is None else TR._oracle(MIXED, funcs[f], (rows[i][0][0],))
           for i, f in enumerate(func_of)]
    lens = [0 if f is None else 2 if f == 2 else 1 for f in func_of]
    return funcs, func_of, rows, ref, lens


def _rows3(ctx):
    return TR._rows(ctx, 2)


def _check_mixed(ctx, ref, lens, out):
    got = [r[2][:lens[i]] if r[0] == 0 else [] for i, r in enumerate(out)]
    assert compare(ref, got, [r[0] for r in out], [r[1] for r in out], ctx.memory_hash(), None, exact=True) == []


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_fork_call_vector(built, n):
    """A call vector with NO_CALL, trapping, two-result and suspended instances, forked:
    a destination whose source sat the call out, trapped or finished is final at once with
    the source's row and never changes; return_lens() and the result types follow the source."""
    from wasmedge_amd import batch
    funcs, func_of, rows, ref, lens = _mixed_vector(n)
    s = 1000
    ctx = TR._ctx(MIXED, n, max_steps=s)
    try:
        ctx.set_calls(funcs, func_of, rows)
        ctx.run()
        k = _to(ctx, s, 1, 3)
        rec = _rows3(ctx)
        assert {r[0] for r in rec} == {0, 0x89, SUSPENDED}
        assert [int(x) for x in ctx.return_lens()] == lens
        types = ctx.results(2)[0]["type"].tolist()
        snap = ctx.snapshot(invocation=True)
        assert snap.suspended == _nsusp(rec)
        cap = TR._cap(ref, s)
        _, out = _go(ctx, s, k, cap, 2)
        _check_mixed(ctx, ref, lens, out)
        maps = {"identity": None, "reverse": [n - 1 - i for i in range(n)],
                "random": [int(x) for x in np.random.RandomState(3 * n).randint(0, n, n)],
                "shift": [(i + 1) % n for i in range(n)]}
        for name, src in maps.items():
            if name == "random":   # another staging in between: one function, no results
                ctx.set_args("boom", batch.make_values([[1]] * n, [I32]))
                ctx.run()
            ctx.restore(snap, src)
            ident = src or list(range(n))
            assert ctx.suspended() == _nsusp(rec, ident), name
            assert _rows3(ctx) == _mapped(rec, ident), name
            mlens = _mapped(lens, ident)
            assert [int(x) for x in ctx.return_lens()] == mlens, name
            assert ctx.results(2)[0]["type"].tolist() == _mapped(types, ident), name
            final = {i: rec[j] for i, j in enumerate(ident) if rec[j][0] != SUSPENDED}

            def each(k, cur):
                for i, r in final.items():
                    assert cur[i] == r, (name, k, i)
                assert [int(x) for x in ctx.return_lens()] == mlens

            _, out = _go(ctx, s, k, cap, 2, each)
            _check_mixed(ctx, _mapped(ref, ident), mlens, out)
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_deep_stack(built, n):
    """sum(3000 + i), 12 instructions a level, 8 of them on the way down, 2 call-stack cells a
    level: after slice 3 (>= 10821 instructions) an instance is some 1350 levels down, past
    the LDS slots; the 4096 cells are reached near 16400 instructions and the stack doubles;
    after slice 6 (>= 21642) the instance is some 2700 levels down and holds over 5000 cells.
    What a capture holds shows it: the bytes an invocation adds are the frame-save rows (at
    most 158 a wave: the LDS share), 17 bytes an instance (under 5 rows a wave) and the call-stack rows, so more
    than 4096 + 170 rows a wave means a wave holds rows past the first depth.
    Restores: the late capture after a Reset gave the growth back; the early one into the
    stack grown since; a broadcast of the deepest instance."""
    rows = [[3000 + i] for i in range(n)]
    ref = TR._ref(SUM, "sum", rows)
    s, nw = 3607, (n + 63) // 64
    assert 8 * s < ref[0][2] < 12 * s and ref[1][2] - ref[0][2] == 12
    ctx = TR._ctx(SUM, n, max_steps=s)
    try:
        TR._start(ctx, "sum", rows, [I32])
        _to(ctx, s, 1, 3)
        rec3 = TR._rows(ctx, 1)
        assert ctx.suspended() == n
        plain, early = ctx.snapshot(), ctx.snapshot(invocation=True)
        held3 = (early.nbytes - plain.nbytes) / 256 / nw
        plain.close()
        assert 170 < held3 < 4096, held3
        _to(ctx, s, 3, 6)
        rec6 = TR._rows(ctx, 1)
        assert ctx.suspended() == n
        plain, late = ctx.snapshot(), ctx.snapshot(invocation=True)
        held6 = (late.nbytes - plain.nbytes) / 256 / nw
        plain.close()
        assert held6 > 4096 + 170, held6
        cap = TR._cap(ref, s)
        ctx.reset()
        ctx.restore(late)
        assert TR._rows(ctx, 1) == rec6 and ctx.suspended() == n
        _, out = _go(ctx, s, 6, cap, 1)
        TR._final(ctx, ref, out, [I32])
        ctx.restore(early)   # (the stack is the doubled one now)
        assert TR._rows(ctx, 1) == rec3 and ctx.suspended() == n
        _, out = _go(ctx, s, 3, cap, 1)
        TR._final(ctx, ref, out, [I32])
        ctx.reset()
        ctx.restore(late, [n - 1] * n)
        assert TR._rows(ctx, 1) == [rec6[n - 1]] * n
        _, out = _go(ctx, s, 6, cap, 1)
        TR._final(ctx, [ref[n - 1]] * n, out, [I32])
        early.close()
        late.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_memory(built, n):
    """Stores and a memory.grow: captured mid-run, finished, restored and finished again,
    hashes and sizes are the oracle's; a reversal fork takes the sources' memories along."""
    rows = [[40 + i % 9, 64 * (i % 100)] for i in range(n)]
    ref = TR._ref(MEM, "fill", rows)
    s = 101
    ctx = TR._ctx(MEM, n, max_steps=s)
    try:
        TR._start(ctx, "fill", rows, [I32, I32])
        k = _to(ctx, s, 1, 3)
        rec = TR._rows(ctx, 1)
        assert ctx.suspended() == n
        pages = [ctx.memory_pages(i) for i in range(n)]
        snap = ctx.snapshot(invocation=True)
        cap = TR._cap(ref, s)
        for src in (None, None, [n - 1 - i for i in range(n)]):
            if src is None:
                _, out = _go(ctx, s, k, cap, 1)
                TR._final(ctx, ref, out, [I32])
                assert [ctx.memory_pages(i) for i in range(n)] == [2] * n
            ctx.restore(snap, src)
            ident = src or list(range(n))
            assert TR._rows(ctx, 1) == _mapped(rec, ident)
            assert [ctx.memory_pages(i) for i in range(n)] == _mapped(pages, ident)
        _, out = _go(ctx, s, k, cap, 1)
        TR._final(ctx, _mapped(ref, ident), out, [I32])
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_restore_then_feed(built, n):
    """Instances spin on a word of their memory. A restore brings back the memory of the
    capture (the word unwritten) with the instances waiting; what the host writes after the
    restore is what an instance sees when it continues."""
    from wasmedge_amd import batch
    word = [0x1000 + i for i in range(n)]
    data = np.array(word, "<u4").view(np.uint8).reshape(n, 4)
    other = np.array([0x2000 + i for i in range(n)], "<u4").view(np.uint8).reshape(n, 4)
    ctx = TR._ctx(WAIT, n, max_steps=5000)
    try:
        ctx.set_args("wait", np.zeros((n, 0), batch.VALUE_DTYPE))
        ctx.run()
        assert ctx.suspended() == n
        rec = TR._rows(ctx, 1)
        snap = ctx.snapshot(invocation=True)
        assert snap.suspended == n
        assert not ctx.write_memories(other).any()
        ctx.resume(10000)
        assert ctx.suspended() == 0 and [r[2][0] for r in TR._rows(ctx, 1)] == [0x2000 + i for i in range(n)]
        ctx.restore(snap)
        assert ctx.suspended() == n and TR._rows(ctx, 1) == rec
        assert not ctx.write_memories(data, lens=[4 * (1 - i % 2) for i in range(n)]).any()
        ctx.resume(10000)
        rows = TR._rows(ctx, 1)
        for i, r in enumerate(rows):
            if i % 2:
                assert r[0] == SUSPENDED and r[1] >= 10000 and r[2] == [0], (i, r)
            else:
                assert r[0] == 0 and r[2] == [word[i]], (i, r)
        assert ctx.suspended() == n // 2
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_host_imports(built, n):
    """A host call every iteration: after restore and finish the results are the oracle's and
    each instance's host function ran again exactly (calls from the capture to the end) times."""
    from hostfuncs import add_i64
    rows = [[3 + (i * 5) % 17] for i in range(n)]
    ref = TR._ref(HOSTLOOP, "acc", rows)
    calls = {}

    def counted(mem, a):
        calls[mem.instance] = calls.get(mem.instance, 0) + 1
        return add_i64(mem, a)

    s = 37
    ctx = TR._ctx(HOSTLOOP, n, max_steps=s)
    try:
        ctx.add_host_function("env", "add_i64", counted, 2, 1)
        TR._start(ctx, "acc", rows, [I32])
        k = _to(ctx, s, 1, 3)
        before = dict(calls)
        nsusp = ctx.suspended()
        assert 0 < nsusp
        snap = ctx.snapshot(invocation=True)
        cap = TR._cap(ref, s)
        _, out = _go(ctx, s, k, cap, 1)
        TR._final(ctx, ref, out, [I64])
        assert calls == {i: rows[i][0] for i in range(n)}
        rest = {i: rows[i][0] - before.get(i, 0) for i in range(n) if rows[i][0] > before.get(i, 0)}
        assert rest
        calls.clear()
        ctx.restore(snap)
        assert ctx.suspended() == nsusp
        _, out = _go(ctx, s, k, cap, 1)
        TR._final(ctx, ref, out, [I64])
        assert calls == rest
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_gpu_metered(built, n):
    """A cost limit between fib(13)'s and fib(14)'s cost; the odd instances spent fib(12)'s
    cost in an earlier invocation, so they reach the limit (0x03) while even ones still run:
    the capture holds finished, 0x03 and suspended instances. Gas totals after restore and
    finish are the uninterrupted run's; a 0x03 source forked onto a lane leaves it at 0x03."""
    rows = [[10 + i % 7] for i in range(n)]
    limit = (TR._oracle(FIB, "fib", (13,))[2] + TR._oracle(FIB, "fib", (14,))[2]) // 2
    m = O.Module(FIB)
    insts = [O.Instance(m, cost_limit=limit) for _ in range(n)]
    for i in range(1, n, 2):
        assert insts[i].invoke("fib", [12])[0] == 0
    ref = [x.invoke("fib", r) for x, r in zip(insts, rows)]
    costs = [x.cost_sum() for x in insts]
    s, k0 = 1000, 8
    ctx = TR._ctx(FIB, n, max_steps=s, cost_limit=limit)
    try:
        ctx.set_calls(["fib"], [0 if i % 2 else None for i in range(n)], [[(12, I32)]] * n)
        ctx.run()
        _go(ctx, s, 1, 8, 1)
        TR._start(ctx, "fib", rows, [I32])
        k = _to(ctx, s, 1, k0)
        rec = TR._rows(ctx, 1)
        assert {r[0] for r in rec} == {0, 0x03, SUSPENDED}
        snap = ctx.snapshot(invocation=True)
        cap = TR._cap(ref, s)
        _, out = _go(ctx, s, k, cap, 1)
        TR._final(ctx, ref, out, [I32])
        assert {r[0] for r in ref} == {0, 0x03}
        assert [int(c) for c in ctx.total_costs()] == costs
        ctx.restore(snap)
        assert TR._rows(ctx, 1) == rec
        _, out = _go(ctx, s, k, cap, 1)
        TR._final(ctx, ref, out, [I32])
        assert [int(c) for c in ctx.total_costs()] == costs
        src = [int(x) for x in np.random.RandomState(n + 1).randint(0, n, n)]
        gone = [i for i in range(n) if rec[src[i]][0] == 0x03]
        assert gone and any(rec[j][0] == SUSPENDED for j in src)
        ctx.restore(snap, src)
        assert TR._rows(ctx, 1) == _mapped(rec, src)
        _, out = _go(ctx, s, k, cap, 1)
        assert all(out[i] == rec[src[i]] for i in gone)
        TR._final(ctx, _mapped(ref, src), out, [I32])
        assert [int(c) for c in ctx.total_costs()] == _mapped(costs, src)
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_lifecycle(built):
    """When an invocation capture is legal, what its restore allows, and that a plain snapshot
    taken at the same moment still restores to "not parked"."""
    from wasmedge_amd import batch
    n = 65
    rows = _fib_rows(n)
    ref = TR._ref(FIB, "fib", rows)
    vals = batch.make_values(rows, [I32])
    cap = TR._cap(ref, FIB_S)

    def refused(f):
        with pytest.raises(batch.WasmEdgeError) as e:
            f()
        assert e.value.code == 0x04

    plain = TR._ctx(FIB, n, max_steps=FIB_S, resumable=False)
    try:
        plain.set_args("fib", vals)
        plain.run()
        refused(lambda: plain.snapshot(invocation=True))
        plain.snapshot().close()
    finally:
        plain.close()

    ctx = TR._ctx(FIB, n, max_steps=FIB_S)
    try:
        refused(lambda: ctx.snapshot(invocation=True))      # before the first run
        ctx.set_args("fib", vals)
        refused(lambda: ctx.snapshot(invocation=True))
        ctx.run()
        ctx.reset()
        refused(lambda: ctx.snapshot(invocation=True))      # after reset()
        ctx.set_args("fib", vals)
        ctx.run()
        ctx.set_args("fib", vals)
        refused(lambda: ctx.snapshot(invocation=True))      # after set_args
        ctx.run()
        ctx.resume(FIB_K * FIB_S)
        rec, nsusp = TR._rows(ctx, 1), ctx.suspended()
        assert 0 < nsusp < n
        snap, bare = ctx.snapshot(invocation=True), ctx.snapshot()
        assert snap.suspended == nsusp and bare.suspended == 0 and snap.nbytes > bare.nbytes
        # the plain one: not parked, no results, no resume
        ctx.restore(bare)
        assert ctx.suspended() == 0
        refused(lambda: ctx.resume(0))
        refused(lambda: ctx.results(1))
        refused(lambda: ctx.snapshot(invocation=True))
        # the invocation comes back after that, after a reset and after a run of another kind
        for spoil in (lambda: None, ctx.reset, lambda: (ctx.set_calls(["fib"], [0] * n, [[(3, I32)]] * n), ctx.run())):
            spoil()
            ctx.restore(snap)
            assert ctx.suspended() == nsusp and TR._rows(ctx, 1) == rec
            again = ctx.snapshot(invocation=True)           # live again: a capture is legal
            assert again.suspended == nsusp
            again.close()
            _, out = _go(ctx, FIB_S, FIB_K, cap, 1)
            TR._final(ctx, ref, out, [I32])
        # with nothing suspended: legal; its restore makes the results readable, resume launches nothing
        done = ctx.snapshot(invocation=True)
        assert done.suspended == 0
        ctx.reset()
        refused(lambda: ctx.results(1))
        ctx.restore(done)
        assert TR._rows(ctx, 1) == out and ctx.suspended() == 0
        assert ctx.resume(0) == 0.0 and TR._rows(ctx, 1) == out
        # what ends a reinstated invocation
        ctx.restore(snap)
        ctx.set_args("fib", vals)
        refused(lambda: ctx.resume(0))
        ctx.restore(snap)
        ctx.reset()
        refused(lambda: ctx.resume(0))
        # an identity restore under the same staging leaves a run possible: from the top
        ctx.set_args("fib", vals)
        ctx.run()
        early = ctx.snapshot(invocation=True)
        ctx.resume(2 * FIB_S)
        ctx.restore(early)
        ctx.run()
        assert ctx.suspended() == n
        _, out = TR._slices(ctx, FIB_S, cap, 1)
        TR._final(ctx, ref, out, [I32])
        early.close()
        snap.close()              # before the context
    finally:
        ctx.close()
    bare.close()                  # ... and after it
    done.close()
    assert bare.nbytes == 0


@pytest.mark.gpu
@pytest.mark.parametrize("partition", [0, 1])
def test_gpu_shards(built, partition):
    """Devices = [0, 0]: an identity rewind of both shards is oracle-exact; a source map is
    refused with 0x02 and leaves a state that still finishes correctly."""
    from wasmedge_amd import batch
    n = 130
    ctx, ref = _fib_state(n, devices=[0, 0], partition=partition)
    try:
        rec, nsusp = TR._rows(ctx, 1), ctx.suspended()
        assert 0 < nsusp < n
        snap = ctx.snapshot(invocation=True)
        assert snap.suspended == nsusp
        cap = TR._cap(ref, FIB_S)
        _, a = _go(ctx, FIB_S, FIB_K, cap, 1)
        TR._final(ctx, ref, a, [I32])
        ctx.restore(snap)
        assert ctx.suspended() == nsusp and TR._rows(ctx, 1) == rec
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.restore(snap, [n - 1 - i for i in range(n)])
        assert e.value.code == 0x02
        assert ctx.suspended() == nsusp and TR._rows(ctx, 1) == rec
        _, b = _go(ctx, FIB_S, FIB_K, cap, 1)
        assert b == a
        TR._final(ctx, ref, b, [I32])
        snap.close()
    finally:
        ctx.close()
