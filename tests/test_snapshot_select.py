"""Selective restore: WasmEdge_BatchSnapshotRestoreSelected / RestoreSelectedDevice restart
some instances from a snapshot and leave the others (SrcOf[i] == KEEP) exactly as they are.

Expected values come only from the oracle twins of tests/test_snapshot.py: a kept twin is left
alone, a restored twin i is rebuilt as init(seeds[SrcOf[i]]). Every instance is compared:
status, returns, counts, memory hash, pages, both globals, and the table through sum().
130 instances: two full waves and a partial one.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from helpers import compare
from test_args_device import Dev
from test_snapshot import (GRANULES, I32, N, NONE, PLAIN_WAT, SEEDS, XS, XS2, Twins, check, context, gpu_call,
                           src_vectors, wasm)
from wasmedge_amd.wat import assemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wasmedge_amd", "csrc")
KEEP = 0xFFFFFFFF


def keep_vectors():
    """None: the instance is kept"""
    rng = np.random.RandomState(17)
    kept = rng.rand(N) < 0.3
    srcs = src_vectors()["random"]   # (seeded, in [0, N / 2))
    return {
        "none": list(range(N)),
        "all": [None] * N,
        "waves": [i if i < 64 else None if i < 128 else None if i == 128 else i for i in range(N)],
        "waves2": [i if i < 64 else None if i < 128 else i if i == 128 else None for i in range(N)],
        "alternate": [None if i & 1 else i for i in range(N)],
        "fork": [None if kept[i] else srcs[i] for i in range(N)],
        "bcast": [None if i % 4 == 0 else 65 for i in range(N)],
    }


VECTORS = keep_vectors()


def words(m):
    return np.array([KEEP if s is None else s for s in m], np.uint32)


def selected(live, m, build=None):
    """the twins after a selective restore through m: a kept instance is `live`'s, left alone;
    a restored one is rebuilt from its source's seed (build: seeds -> Twins, init alone by
    default)"""
    seeds = [SEEDS[i if s is None else s] for i, s in enumerate(m)]
    tw = build(seeds) if build else Twins(seeds, **live.kw)
    tw.inst = [live.inst[i] if s is None else tw.inst[i] for i, s in enumerate(m)]
    return tw


def restore_device(ctx, snap, arr, timed=True):
    """the Device entry with a buffer the bound HIP runtime allocated; (seconds, restored)"""
    from wasmedge_amd import batch
    d = Dev(np.ascontiguousarray(arr, np.uint32))
    try:
        t, r = ctypes.c_double(0), ctypes.c_uint32(0)
        ctx._check(batch.lib().WasmEdge_BatchSnapshotRestoreSelectedDevice(ctx._h, snap._h, d.ptr, ctypes.byref(r),
                                                                           ctypes.byref(t) if timed else None))
        return t.value, int(r.value)
    finally:
        d.free()


def refused(fn, code, text=None):
    from wasmedge_amd import batch
    with pytest.raises(batch.WasmEdgeError) as e:
        fn()
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value)


# ---- CPU cases ----------------------------------------------------------------------------
def test_header_compiles_as_c(built, tmp_path):
    src = tmp_path / "select_abi.c"
    src.write_text('#include "wasmedge_batch.h"\n'
                   "WasmEdge_Result some(WasmEdge_BatchContext *c, const WasmEdge_BatchSnapshot *s, const uint32_t *m,\n"
                   "                     uint32_t *n, double *t) {\n"
                   "  if (m && m[0] == WASMEDGE_BATCH_SNAPSHOT_KEEP) return WasmEdge_BatchSnapshotRestoreSelected(c, s, m, n, t);\n"
                   "  return WasmEdge_BatchSnapshotRestoreSelectedDevice(c, s, m, n, t); }\n")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "select_abi.o")])


def test_null_arguments(built):
    """through ctypes on the product library, no GPU touched"""
    from wasmedge_amd import batch
    L = batch.lib()
    assert L.WasmEdge_BatchSnapshotRestoreSelected(None, None, None, None, None).Code == 0x04
    assert L.WasmEdge_BatchSnapshotRestoreSelectedDevice(None, None, None, None, None).Code == 0x04


def test_restore_tensor_refuses_before_the_library(built):
    """a non-tensor, a wrong dtype and a wrong shape: ValueError from a context that has no
    handle, so no library call can have happened"""
    import torch
    from wasmedge_amd import batch
    ctx = batch.BatchContext.__new__(batch.BatchContext)
    ctx.n = N
    snap = batch.Snapshot(None)
    for bad in ([0] * N, np.zeros(N, np.int32), torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.uint8),
                torch.zeros(N - 1, dtype=torch.int32), torch.zeros((N, 1), dtype=torch.int32),
                torch.zeros(N, dtype=torch.int32)):   # (the last: not on the device)
        with pytest.raises(ValueError):
            ctx.restore_tensor(snap, bad)
    with pytest.raises(ValueError):
        ctx.restore_selected(snap, [0] * N)   # (a closed snapshot)


PLAN_MAIN = r"""
#include <stdio.h>
#include "snapshot_plan.h"
// stdin: n same_granule, nwaves rows, n sources; stdout: per wave class, keep flag and tiles,
// the source of every lane, then max_tiles identity any_keep restored
int main() {
  unsigned n, same;
  if (scanf("%u %u", &n, &same) != 2) return 2;
  const unsigned nw = (n + 63) / 64;
  std::vector<uint32_t> rows(nw), src(n);
  for (auto &r : rows) if (scanf("%u", &r) != 1) return 2;
  for (auto &s : src) if (scanf("%u", &s) != 1) return 2;
  wbs::RestorePlan P;
  wbs::plan_restore(src.data(), n, nw, rows.data(), same != 0, &P);
  for (unsigned w = 0; w < nw; w++)
    printf("%u %u %u\n", P.wave[2 * w] & wbs::kClassMask, P.wave[2 * w] & wbs::kHasKeep ? 1 : 0, P.wave[2 * w + 1]);
  for (unsigned i = 0; i < nw * 64; i++) printf("%u\n", P.src[i]);
  printf("%u %d %d %u\n", P.max_tiles, P.identity ? 1 : 0, P.any_keep ? 1 : 0, P.restored);
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("select_plan")
    (d / "main.cpp").write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "main.cpp"), "-o",
                           str(d / "plan")])
    return str(d / "plan")


@pytest.mark.parametrize("name", sorted(VECTORS))
@pytest.mark.parametrize("same", [1, 0])
def test_plan_against_model(plan_prog, name, same):
    """class and keep flag of every wave, tiles over restored lanes only, the source of every
    lane of the padded last wave, identity and max_tiles against a brute-force model"""
    m = VECTORS[name]
    nw = (N + 63) // 64
    rows = [192, 2304, 64]
    text = "%d %d\n%s\n%s\n" % (N, same, " ".join(map(str, rows)), " ".join(str(int(x)) for x in words(m)))
    out = subprocess.run([plan_prog], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    lanes = []
    for i in range(nw * 64):   # a lane past n follows lane 0 of its wave, kept when that is
        lead = m[i & ~63]
        lanes.append(m[i] if i < N else None if lead is None else (lead & ~63) | (i & 63))
    biggest, ident = 0, True
    for w in range(nw):
        mine = lanes[w * 64:(w + 1) * 64]
        rest = [(w * 64 + l, s) for l, s in enumerate(mine) if s is not None]
        if not rest:
            cls, flag, tiles = 3, 0, 0
        else:
            waves = {s >> 6 for _, s in rest}
            cls = 0 if same and all(i == s for i, s in rest) else 1 if len(waves) == 1 else 2
            flag = 1 if len(rest) < 64 else 0
            tiles = max(rows[v] for v in waves) // 64
        assert out[w].split() == [str(cls), str(flag), str(tiles)], (w, out[w])
        biggest = max(biggest, tiles)
        ident = ident and (cls == 3 or (cls == 0 and not flag))
    assert [int(v) for v in out[nw:nw + nw * 64]] == [KEEP if s is None else s for s in lanes]
    kept = sum(1 for s in m if s is None)
    assert out[nw + nw * 64].split() == [str(biggest), "1" if ident else "0", "1" if kept else "0", str(N - kept)]


def test_rehearsal_of_the_kernel_bodies(tmp_path):
    """tests/c/snapshot_rehearsal.cpp: the memory-0 restore, the rows kernel and the plan kernel
    as host code under the address and undefined-behaviour sanitizers, a thread per GPU thread,
    against a per-lane word model -- every keep vector, granules 4, 8, 16 and 128, the layout
    of the capture, a doubled one and a changed granule. No report, no differing word."""
    exe = str(tmp_path / "rehearsal")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-pthread", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "snapshot_rehearsal.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)   # (well under a minute)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ---- GPU cases ----------------------------------------------------------------------------
def stepped(ctx, snap, first):
    """the state every case starts from: init(SEEDS) (the snapshot), then step(XS)"""
    if not first:
        ctx.restore(snap)
    gpu_call(ctx, "step", XS, 1)
    live = Twins(SEEDS)
    live.call("step", XS)
    return live


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_parity(built, granule):
    """init, snapshot, step, restore_selected(map): sum, a second step and sum again, for
    every keep vector"""
    ctx = context(granule)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    for k, (name, m) in enumerate(VECTORS.items()):
        live = stepped(ctx, snap, k == 0)
        before = ctx.memory_hash()
        _, restored = ctx.restore_selected(snap, m)
        assert restored == sum(1 for s in m if s is not None), name
        with pytest.raises(Exception):   # results are as after a restore: none until a run
            ctx.results(1)
        if name == "all":
            assert restored == 0 and (ctx.memory_hash() == before).all()
        if name == "none":   # exactly what restore(snap) leaves
            mine = ctx.memory_hash()
            ctx.restore(snap)
            assert (ctx.memory_hash() == mine).all()
        tw = selected(live, m)
        check(ctx, tw, "sum", NONE, 1, name)
        check(ctx, tw, "step", XS2, 1, name)
        check(ctx, tw, "sum", NONE, 1, name + " again")
    snap.close()
    ctx.close()


def fresh_again(ctx, what):
    """after a Reset every instance is a fresh one: the write marks covered everything; a
    fresh page reads zero"""
    ctx.reset()
    tw = Twins()
    check(ctx, tw, "init", SEEDS, 0, what)
    check(ctx, tw, "step", XS, 1, what)
    check(ctx, tw, "growsum", NONE, 1, what)


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [4, 128])
def test_marks_stay_sound(built, granule):
    """kept lanes with high marks and wide tables beside restored lanes with low ones, and
    the converse; after each: sum, then reset() and fresh twins"""
    m = VECTORS["fork"]
    ctx = context(granule)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    _, st, _ = gpu_call(ctx, "scribble", NONE, 0)
    assert not st.any()
    live = Twins(SEEDS)
    live.call("scribble", NONE)
    ctx.restore_selected(snap, m)
    for i, s in enumerate(m):   # a kept lane's widened table survives; a restored one's is its source's
        if i in (0, 1, 2, 63, 64, 65, 127, 128, 129):
            want = 4 + (SEEDS[s][0] % 6 if SEEDS[s][0] % 3 == 0 else 0) if s is not None else None
            assert (ctx.table_size("t", i) > 5000) if s is None else (ctx.table_size("t", i) == want), i
            assert ctx.memory_pages(i) == (8 if s is None else 2 if SEEDS[s][0] % 5 == 0 else 1), i
    check(ctx, selected(live, m), "sum", NONE, 1, "high marks kept")
    fresh_again(ctx, "after high marks kept")
    snap.close()
    # the converse: the snapshot holds the scribbled state, the lanes the small one
    ctx.reset()
    gpu_call(ctx, "init", SEEDS, 0)
    gpu_call(ctx, "scribble", NONE, 0)
    snap = ctx.snapshot()
    ctx.reset()
    gpu_call(ctx, "init", SEEDS, 0)

    def scribbled(seeds):
        tw = Twins(seeds)
        tw.call("scribble", NONE)
        return tw

    ctx.restore_selected(snap, m)
    check(ctx, selected(Twins(SEEDS), m, scribbled), "sum", NONE, 1, "high marks restored")
    fresh_again(ctx, "after high marks restored")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_pool_rows(built, monkeypatch):
    """kept instances hold pool rows: with the layout pinned the restore fails with 0x02 and
    the capture's message and nothing changed; unpinned the layout takes the rows first"""
    m = VECTORS["alternate"]
    monkeypatch.setenv("WB_RELAYOUT", "0")
    ctx = context(4, memory_reserve_pages=2)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    live = Twins(SEEDS)
    check(ctx, live, "scribble", NONE, 0, "scribble")
    assert ctx.reserved_pages() == 2
    check(ctx, live, "sum", NONE, 1, "before")
    refused(lambda: ctx.restore_selected(snap, m), 0x02, "reserved layout")
    check(ctx, live, "sum", NONE, 1, "after the refused restore")
    monkeypatch.delenv("WB_RELAYOUT")
    _, restored = ctx.restore_selected(snap, m)
    assert restored == N // 2 and ctx.reserved_pages() >= 8
    assert all(ctx.memory_pages(i) == 8 for i in range(1, N, 2))
    tw = selected(live, m)
    check(ctx, tw, "sum", NONE, 1, "the kept lanes' 8 pages")
    check(ctx, tw, "step", XS, 1, "step")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_deferred_reset(built):
    """a Reset left to the next launch is carried out for the kept lanes, not cancelled"""
    from wasmedge_amd import batch
    m = VECTORS["alternate"]
    w = assemble(PLAIN_WAT)
    mod = O.Module(w)
    ctx = batch.BatchContext(w, N, device=0, memory_granule=4)

    def both(twins, func, rows, nret, what):
        exp = [t.invoke(func, r) for t, r in zip(twins, rows)]
        rets, st, cnt = gpu_call(ctx, func, rows, nret)
        bad = compare(exp, rets, st, cnt, ctx.memory_hash(), [I32] * nret, exact=True)
        assert not bad, (what, bad[:5])

    tw = [O.Instance(mod) for _ in range(N)]
    both(tw, "fill", SEEDS, 0, "fill")
    snap = ctx.snapshot()
    gpu_call(ctx, "fill", XS, 0)
    ctx.reset(timed=False)
    ctx.restore_selected(snap, m, timed=False)
    tw = [O.Instance(mod) if s is None else tw[s] for s in m]   # kept: fresh; restored: its source
    both(tw, "sum", NONE, 1, "sum after untimed reset + selective restore")
    both(tw, "fill", XS2, 0, "fill after it")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_multi_memories(built):
    """memories 1 and 2 and their sizes are kept and restored per lane"""
    from test_multimem import MM_WAT
    from wasmedge_amd import batch
    m = VECTORS["fork"]
    w = assemble(MM_WAT)
    mod = O.Module(w, multi_memory=True)
    rows = [[i * 3 + 1, 20 + i % 40] for i in range(N)]
    rows2 = [[i * 5 + 2, 10 + i % 30] for i in range(N)]
    rows3 = [[i * 7 + 3, 15 + i % 20] for i in range(N)]
    ctx = batch.BatchContext(w, N, device=0, multi_memory=True)
    ctx.execute("run", batch.make_values(rows, [I32, I32]), 1)
    snap = ctx.snapshot()
    ctx.execute("run", batch.make_values(rows2, [I32, I32]), 1)
    ctx.restore_selected(snap, m)
    tw = [O.Instance(mod) for _ in range(N)]
    for i, (t, s) in enumerate(zip(tw, m)):
        t.invoke("run", rows[i if s is None else s])
        if s is None:
            t.invoke("run", rows2[i])
    exp = [t.invoke("run", r) for t, r in zip(tw, rows3)]
    rets, st, cnt = gpu_call(ctx, "run", rows3, 1)
    assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True) == []
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_metered(built):
    """the gas total of a kept lane keeps running; a restored lane takes its source's"""
    m = VECTORS["fork"]
    limit = 60000
    ctx = context(4, cost_limit=limit)
    live = Twins(cost_limit=limit)
    check(ctx, live, "init", SEEDS, 0, "init")
    at_capture = [t.cost_sum() for t in live.inst]
    snap = ctx.snapshot()
    check(ctx, live, "step", XS, 1, "step")
    ctx.restore_selected(snap, m)
    tw = selected(live, m)
    want = [live.inst[i].cost_sum() if s is None else at_capture[s] for i, s in enumerate(m)]
    assert [int(c) for c in ctx.total_costs()] == want
    st = check(ctx, tw, "sum", NONE, 1, "sum: some instances run out of gas")
    assert (st == 0x03).any() and (st == 0).any()
    assert [int(c) for c in ctx.total_costs()] == [t.cost_sum() for t in tw.inst]
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_wasi_lane_state(built):
    """a kept lane keeps its captured output, exit code and fd table, a restored one has its
    source's (instance 3's); index and own argv stay. Host map and device map alike."""
    from test_wasi import ARGS, ENVS, WASI
    from wasmedge_amd import batch
    n = 96
    r1 = [[x] for x in range(n)]
    r2 = [[(x * 5 + 8) % 96] for x in range(n)]
    r3 = [[(x * 7) % 96] for x in range(n)]
    own = {7: ["seven", "x"], 40: ["forty"], 41: ["forty-one"]}
    m = [None if i & 1 else 3 for i in range(n)]
    ctx = batch.BatchContext(WASI, n, device=0)
    ctx.init_wasi(ARGS, ENVS)
    for i, a in own.items():
        ctx.set_instance_args(i, a)
    O.set_wasi(True, ARGS, ENVS)
    try:
        mod = O.Module(WASI)

        def twins():
            """kept: its own two runs; restored: instance 3's first run, own argv from then on"""
            tw = [O.Instance(mod) for _ in range(n)]
            for i, t in enumerate(tw):
                if m[i] is None and i in own:
                    t.set_args(own[i])
                t.invoke("run", r1[i] if m[i] is None else r1[3])
                if m[i] is None:
                    t.invoke("run", r2[i])
                elif i in own:
                    t.set_args(own[i])
            return tw

        def side(tw):
            return [(t.wasi_output(1), t.wasi_output(2), t.wasi_exit_code()) for t in tw]

        def gpu_side():
            return [(ctx.wasi_output(i, 1), ctx.wasi_output(i, 2), ctx.wasi_exit_code(i)) for i in range(n)]

        gpu_call(ctx, "run", r1, 1)
        snap = ctx.snapshot()
        seen = []
        for device in (False, True):
            gpu_call(ctx, "run", r2, 1)
            if device:
                _, restored = restore_device(ctx, snap, words(m))
            else:
                _, restored = ctx.restore_selected(snap, m)
            assert restored == n // 2
            tw = twins()
            assert gpu_side() == side(tw), device
            exp = [t.invoke("run", r) for t, r in zip(tw, r3)]
            rets, st, cnt = gpu_call(ctx, "run", r3, 1)
            assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True) == [], device
            assert gpu_side() == side(tw), device
            seen.append((gpu_side(), [int(h) for h in ctx.memory_hash()]))
            ctx.restore(snap)
        assert seen[0] == seen[1]
    finally:
        O.set_wasi(False)
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_suspended_snapshot(built):
    """a snapshot that holds an invocation: any KEEP gives 0x04 through both entries and the
    live run continues bit-exactly; a fork without KEEP equals restore(snap, src_of) through
    both entries"""
    import test_resume as TR
    import test_snapshot_suspended as TS
    ctx, ref = TS._fib_state(N)
    try:
        rec = TR._rows(ctx, 1)
        snap = ctx.snapshot(invocation=True)
        cap = TR._cap(ref, TS.FIB_S)
        keep = [None if i & 1 else i for i in range(N)]
        refused(lambda: ctx.restore_selected(snap, keep), 0x04, "invocation")
        refused(lambda: restore_device(ctx, snap, words(keep)), 0x04, "invocation")
        assert TR._rows(ctx, 1) == rec
        _, out = TS._go(ctx, TS.FIB_S, TS.FIB_K, cap, 1)
        TR._final(ctx, ref, out, [I32])
        src = [int(x) for x in np.random.RandomState(N).randint(0, N, N)]
        ends = []
        for how in ("restore", "selected", "device"):
            if how == "restore":
                ctx.restore(snap, src)
            elif how == "selected":
                assert ctx.restore_selected(snap, src)[1] == N
            else:
                assert restore_device(ctx, snap, words(src))[1] == N
            assert ctx.suspended() == TS._nsusp(rec, src) and TR._rows(ctx, 1) == TS._mapped(rec, src), how
            _, out = TS._go(ctx, TS.FIB_S, TS.FIB_K, cap, 1)
            TR._final(ctx, TS._mapped(ref, src), out, [I32])
            ends.append((out, [int(h) for h in ctx.memory_hash()]))
        assert ends[0] == ends[1] == ends[2]
        snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_live_invocation_ends(built):
    """a resumable context with a live suspended invocation, a plain snapshot and kept lanes:
    the invocation ends and a fresh run is right on kept and restored lanes"""
    from wasmedge_amd import batch
    m = VECTORS["alternate"]
    ctx = context(4, resumable=True, max_steps=3000)

    def finish(func, rows):
        ctx.set_args(func, batch.make_values(rows, [I32] * len(rows[0])))
        ctx.run()
        ctx.resume(0)
        assert ctx.suspended() == 0

    finish("init", SEEDS)
    snap = ctx.snapshot()
    finish("step", XS2)
    live = Twins(SEEDS)
    live.call("step", XS2)
    ctx.set_args("sum", batch.make_values(NONE, []))
    ctx.run()
    assert ctx.suspended() == N   # (sum retires far more than 3000 instructions)
    _, restored = ctx.restore_selected(snap, m)
    assert restored == N // 2 and ctx.suspended() == 0
    refused(lambda: ctx.resume(0), 0x04)
    check(ctx, selected(live, m), "step", XS, 1, "a fresh run after the invocation ended")
    snap.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("part", [0, 1])
def test_two_shards(built, part):
    """two shards on one device: a map of KEEP and i is legal and right on both; a fork gives
    0x02 and changes nothing; so does the Device entry"""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, devices=[0, 0], partition=part)

    def both(tw, func, rows, nret, what):
        exp = tw.call(func, rows)
        rets, st, cnt = gpu_call(ctx, func, rows, nret)
        assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32] * nret, exact=True) == [], what

    live = Twins()
    both(live, "init", SEEDS, 0, "init")
    snap = ctx.snapshot()
    both(live, "step", XS, 1, "step")
    before = ctx.memory_hash()
    refused(lambda: ctx.restore_selected(snap, VECTORS["fork"]), 0x02, "multi-device")
    refused(lambda: restore_device(ctx, snap, words(VECTORS["alternate"])), 0x02, "multi-device")
    assert (ctx.memory_hash() == before).all()
    both(live, "sum", NONE, 1, "state untouched by the refused restores")
    _, restored = ctx.restore_selected(snap, VECTORS["alternate"])
    assert restored == N // 2
    tw = selected(live, VECTORS["alternate"])
    both(tw, "sum", NONE, 1, "sum")
    both(tw, "step", XS2, 1, "step")
    ctx.close()
    snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [4, 128])
def test_device_map(built, granule):
    """every vector through a device buffer equals the host entry on hashes, sum and the
    count; an invalid entry gives 0x04 with the state unchanged; a short buffer is refused"""
    ctx = context(granule)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    first = True
    for name, m in VECTORS.items():
        seen = []
        for device in (False, True):
            stepped(ctx, snap, first)
            first = False
            _, restored = restore_device(ctx, snap, words(m)) if device else ctx.restore_selected(snap, m)
            hashes = [int(h) for h in ctx.memory_hash()]
            rets, st, cnt = gpu_call(ctx, "sum", NONE, 1)
            seen.append((restored, hashes, rets, [int(x) for x in st], [int(x) for x in cnt]))
        assert seen[0] == seen[1], name
        assert seen[0][0] == sum(1 for s in m if s is not None), name
    live = stepped(ctx, snap, False)
    for bad in (N, 0xFFFFFFFE):
        arr = words(VECTORS["alternate"])
        arr[77] = bad
        arr[100] = bad
        refused(lambda: restore_device(ctx, snap, arr), 0x04, "instance 77")
        refused(lambda: ctx.restore_selected(snap, [int(x) for x in arr]), 0x04)
        check(ctx, live, "sum", NONE, 1, "state untouched by an invalid map")
    for bad in (2 ** 32 + 3, -7):   # no 32-bit instance: 0x04 from an array and from a list alike
        wide = words(VECTORS["alternate"]).astype(np.int64)
        wide[77] = bad
        refused(lambda: ctx.restore_selected(snap, wide), 0x04)
        refused(lambda: ctx.restore_selected(snap, [int(x) for x in wide]), 0x04)
    check(ctx, live, "sum", NONE, 1, "state untouched by entries past 32 bits")
    refused(lambda: restore_device(ctx, snap, words(VECTORS["alternate"])[:N - 1]), 0x02, "smaller")
    check(ctx, live, "sum", NONE, 1, "state untouched by a short buffer")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_gpu_tensor_mirror(built):
    """tests/snapshot_select_tensor_child.py, once: restore_tensor with an int32 tensor that
    torch.where made from a status tensor, against restore_selected, in a process where torch
    initialises its device before the first context exists"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "snapshot_select_tensor_child.py")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["kept"] > 0 and res["restored"] == N - res["kept"], res
    assert res["restored_equal"] and res["hashes_equal"] and res["sums_equal"] and res["results_gone"], res
