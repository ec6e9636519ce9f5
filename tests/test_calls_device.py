"""Device-resident per-instance calls: WasmEdge_BatchSetCallsDevice stages a call vector from a
device FuncOf and rows of 64-bit slots in device memory, WasmEdge_BatchCallsResultsDevice
writes each instance's results by its own function's signature, with the result counts,
statuses and instruction counts, into device memory (include/wasmedge_batch.h; Python:
set_calls_tensor / calls_results_tensor).

The yardstick is always the host path (set_calls / results / return_lens) on the same context,
which tests/test_calls.py pins to the oracle: device and host must agree bit for bit. Device
buffers come from the HIP runtime the library is bound to (test_args_device.Dev); the tensor
mirror runs once in a process of its own (tests/calls_tensor_child.py). 130 instances: two
full waves and two lanes.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import calls_cases as K
from test_args_device import Dev, last_error
from wasmedge_amd.wat import assemble

I32, I64, F32, F64, V128, EXTERNREF = 0x7F, 0x7E, 0x7D, 0x7C, 0x7B, 0x6F
N = 130
NO_CALL = 0xFFFFFFFF
ONES = 0xFFFFFFFF00000000
ALL1 = 0xFFFFFFFFFFFFFFFF
SENTINEL = 0x5AA55AA55AA55AA5
LEN_FILL = 0x5A5A5A5A
DIV_ZERO, SUSPENDED = 0x84, 0x07

FIB = r"""
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2)))))))"""
# a counted loop beside fib, for the resumable runs
SPIN = assemble("(module" + FIB + r"""
  (func (export "spin") (param $n i32) (result i32)
    (local $i i32) (local $s i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $n)))
      (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (local.get $i)))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.get $s)))
""")
# an export that is itself a host import, and one with an externref parameter
AUX = assemble(r"""(module
  (import "env" "add_i64" (func $add (param i64 i64) (result i64)))
  (export "add" (func $add))""" + FIB + r"""
  (func (export "one") (result i32) (i32.const 1))
  (func (export "xref") (param $r externref) (result externref) (local.get $r)))
""")


def slots_of(types):
    return sum(2 if t == V128 else 1 for t in types)


class Vec:
    """funcs, types (one list per name, or None), func_of (index or None) and rows of
    (value, type) pairs: what set_calls takes, and the device form of the same vector"""

    def __init__(self, funcs, types, func_of, rows):
        self.funcs, self.types, self.func_of, self.rows = funcs, types, list(func_of), [list(r) for r in rows]
        self.n = len(self.func_of)

    def fo(self):
        return np.array([NO_CALL if f is None else f for f in self.func_of], np.uint32)

    def slots(self, extra=2):
        """[n][widest row + extra] uint64: the values from slot 0, all-ones upper halves on
        the 32-bit values, all-ones padding"""
        width = max([slots_of([t for _, t in r]) for r in self.rows] + [0]) + extra
        out = np.full((self.n, max(width, 1)), ALL1, np.uint64)
        for i, r in enumerate(self.rows):
            at = 0
            for v, t in r:
                if t == V128:
                    out[i, at], out[i, at + 1] = v & ALL1, v >> 64
                    at += 2
                else:
                    out[i, at] = (v & ALL1) | (ONES if t in (I32, F32) else 0)
                    at += 1
        return out


IDLE_LANES = (3, 63, 64, 129)
UNKNOWN_LANE, WRONG_TYPES_LANE = 5, 6


def mixed(n):
    """Instance i calls NAMES[i % 7]; NO_CALL at 3, 63, 64 and 129, an unknown name at 5, and
    at 6 a second entry for walk whose ParamTypes row is wrong (i32, i64)"""
    funcs = K.NAMES + ["nosuch", "walk"]
    types = [K.PTYPES[f] for f in K.NAMES] + [[I32], [I32, I64]]
    func_of, rows = [], []
    for i in range(n):
        name = K.NAMES[i % len(K.NAMES)]
        f, row = i % len(K.NAMES), [(v, t) for v, t in zip(K.args_of(name, i), K.PTYPES[name])]
        if i in IDLE_LANES:
            f = None
        elif i == UNKNOWN_LANE:
            f, row = len(K.NAMES), [(1, I32)]
        elif i == WRONG_TYPES_LANE:
            f, row = len(K.NAMES) + 1, [(i * 13 + 1, I32), (2, I64)]
        func_of.append(f)
        rows.append(row)
    return Vec(funcs, types, func_of, rows)


def stage_device(ctx, vec, fo=None, slots=None, stride=None, types="vec", null_fo=False, null_slots=False,
                 slots_off=0, drop_lens=False):
    """WasmEdge_BatchSetCallsDevice on device copies of the vector (uploaded here); its code"""
    from wasmedge_amd import batch
    types = vec.types if types == "vec" else types
    names, arr, tptrs, tlens, keep = batch.call_names(vec.funcs, types)
    slots = vec.slots() if slots is None else slots
    d_fo, d_slots = Dev(vec.fo() if fo is None else fo), Dev(slots)
    try:
        return batch.lib().WasmEdge_BatchSetCallsDevice(
            ctx._h, arr, len(names), tptrs, None if drop_lens else tlens, None if null_fo else d_fo.ptr,
            None if null_slots else d_slots.ptr.value + slots_off, slots.shape[1] if stride is None else stride).Code
    finally:
        d_fo.free()
        d_slots.free()


def stage_host(ctx, vec):
    ctx.set_calls(vec.funcs, vec.func_of, vec.rows)


def read_host(ctx, width):
    """results() and return_lens() as the rows CallsResultsDevice has to write: (slots
    [n][width] with zeroes past each row's values, lens, status, counts)"""
    lens = ctx.return_lens()
    rets, st, cnt = ctx.results(max(int(lens.max()), 1))
    out = np.zeros((ctx.n, width), np.uint64)
    for i in range(ctx.n):
        at = 0
        for k in range(int(lens[i])):
            out[i, at] = rets["lo"][i, k]
            at += 1
            if rets["type"][i, k] == V128:
                out[i, at] = rets["hi"][i, k]
                at += 1
            else:
                assert rets["hi"][i, k] == 0
    return out, lens.copy(), st.copy(), cnt.copy()


def read_device(ctx, width, stride, want_slots=True):
    """WasmEdge_BatchCallsResultsDevice into sentinel-filled device arrays: (code, slots
    [n][stride], lens, status, counts)"""
    from wasmedge_amd import batch
    bufs = [Dev(np.full((ctx.n, stride), SENTINEL, np.uint64)), Dev(np.full(ctx.n, LEN_FILL, np.uint32)),
            Dev(np.full(ctx.n, 0x77, np.uint8)), Dev(np.full(ctx.n, SENTINEL, np.uint64))]
    try:
        code = batch.lib().WasmEdge_BatchCallsResultsDevice(ctx._h, bufs[0].ptr if want_slots else None, width, stride,
                                                            bufs[1].ptr, bufs[2].ptr, bufs[3].ptr).Code
        return (code,) + tuple(b.numpy() for b in bufs)
    finally:
        for b in bufs:
            b.free()


def untouched(got):
    return (got[1] == np.uint64(SENTINEL)).all() and (got[2] == LEN_FILL).all() and (got[3] == 0x77).all() \
        and (got[4] == np.uint64(SENTINEL)).all()


def both_reads_agree(ctx, width, case):
    """CallsResultsDevice (rows two slots wider than Width) against results() / return_lens();
    returns the host quadruple"""
    got = read_device(ctx, width, width + 2)   # (first: it must not lean on the host copy)
    assert got[0] == 0, (case, last_error(ctx))
    want = read_host(ctx, width)
    assert np.array_equal(got[1][:, :width], want[0]), case
    assert (got[1][:, width:] == np.uint64(SENTINEL)).all(), case
    for a, b in zip(got[2:], want[1:]):
        assert np.array_equal(a, b), case
    return want


def same(a, b, case=""):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), case


def calls_ctx(n, **kw):
    from hostfuncs import add_i64
    from wasmedge_amd import batch
    ctx = batch.BatchContext(kw.pop("wasm", K.CALLS), n, device=0, **kw)
    ctx.add_host_function("env", "add_i64", add_i64, 2, 1)
    return ctx


@pytest.fixture(scope="module")
def ctx130(built):
    ctx = calls_ctx(N)
    yield ctx
    ctx.close()


WIDEST_R = max(slots_of(t) for t in K.RTYPES.values())   # mv: a v128 and an f64


# ---- no GPU needed ------------------------------------------------------------------------

def test_symbols_refuse_a_null_context(built):
    from wasmedge_amd import batch
    L = batch.lib()
    names, arr, tptrs, tlens, keep = batch.call_names(["f"], [[I32]])
    assert L.WasmEdge_BatchSetCallsDevice(None, arr, 1, tptrs, tlens, None, None, 1).Code == 0x04
    assert L.WasmEdge_BatchCallsResultsDevice(None, None, 1, 1, None, None, None).Code == 0x04


def test_tensor_arguments_are_checked_before_any_call():
    """What is no contiguous device tensor of the right dtype and shape, and what is no list
    of value types per name, is refused with ValueError before the library is called (the
    context here has no handle at all)."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext.__new__(batch.BatchContext)
    ctx.n, ctx._h = 4, None
    fo, rows = np.zeros(4, np.int32), np.zeros((4, 2), np.int64)
    with pytest.raises(ValueError):
        ctx.set_calls_tensor(["f"], fo, rows)                   # not tensors
    with pytest.raises(ValueError):
        ctx.set_calls_tensor(["f"], None, None)                 # func_of is needed
    with pytest.raises(ValueError):
        ctx.set_calls_tensor(["f"], fo, rows, types=[[0x12]])   # not a value type
    with pytest.raises(ValueError):
        ctx.set_calls_tensor(["f", "g"], fo, rows, types=[[I32]])   # one list per name
    with pytest.raises(ValueError):
        ctx.set_calls_tensor([7], fo, rows)                     # not a name
    with pytest.raises(ValueError):
        ctx.calls_results_tensor(2, out=rows)
    with pytest.raises(ValueError):
        ctx.calls_results_tensor(1, lens=np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        ctx.calls_results_tensor(1, status=np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        ctx.calls_results_tensor(1, counts=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        ctx.calls_results_tensor(-1)
    with pytest.raises(ValueError):
        ctx.calls_results_tensor([I32])


# ---- GPU ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 130])
def test_gpu_mixed_all_four_paths(built, ctx130, n):
    """Host or device staging, host or device results: the four combinations give the same
    values, result counts, statuses and instruction counts, and the same memories."""
    ctx = ctx130 if n == N else calls_ctx(n)
    try:
        vec = mixed(n)
        ctx.reset()
        stage_host(ctx, vec)
        ctx.run()
        host = both_reads_agree(ctx, WIDEST_R + 2, "host staging")
        hh = ctx.memory_hash()
        ctx.reset()
        assert stage_device(ctx, vec) == 0, last_error(ctx)
        ctx.run()
        dev = both_reads_agree(ctx, WIDEST_R + 2, "device staging")
        same(host, dev)
        assert np.array_equal(hh, ctx.memory_hash())
        st = host[2]
        for i, want in [(i, 0) for i in IDLE_LANES] + [(UNKNOWN_LANE, 0x05), (WRONG_TYPES_LANE, 0x83)]:
            if i < n:
                assert int(st[i]) == want and int(host[3][i]) == 0 and int(host[1][i]) == 0, i
        if n == N:
            assert (st == DIV_ZERO).any() and host[0].any()
    finally:
        if ctx is not ctx130:
            ctx.close()


@pytest.mark.gpu
def test_gpu_width_and_stride(built, ctx130):
    """A row gets exactly Width slots -- its function's, then zeroes; all zeroes for a trapped
    instance and one that sat out -- and keeps what it held from Width to Stride."""
    ctx, vec = ctx130, mixed(N)
    ctx.reset()
    assert stage_device(ctx, vec) == 0, last_error(ctx)
    ctx.run()
    width, stride = WIDEST_R + 2, WIDEST_R + 5
    want = read_host(ctx, width)
    got = read_device(ctx, width, stride)
    assert got[0] == 0, last_error(ctx)
    assert np.array_equal(got[1][:, :width], want[0]) and (got[1][:, width:] == np.uint64(SENTINEL)).all()
    same(got[2:], want[1:])
    trapped = want[2] == DIV_ZERO
    assert trapped.any() and not got[1][trapped, :width].any()
    assert not got[1][list(IDLE_LANES), :width].any()
    for i in range(N):   # zeroes after each function's own slots
        name = None if vec.func_of[i] is None else vec.funcs[vec.func_of[i]]
        own = slots_of(K.RTYPES.get(name, [])) if i not in (UNKNOWN_LANE, WRONG_TYPES_LANE) else 0
        assert not got[1][i, own:width].any(), i
    mv = [i for i in range(N) if i % 7 == 4 and i not in IDLE_LANES]
    assert got[1][mv, :WIDEST_R].any(axis=1).all()
    # Width one less than the widest result row: refused, nothing written
    got = read_device(ctx, WIDEST_R - 1, stride)
    assert got[0] == 0x04 and last_error(ctx) and untouched(got)
    got = read_device(ctx, width, width - 1)
    assert got[0] == 0x04 and untouched(got)
    # NULL Slots: lens, statuses and counts alone
    got = read_device(ctx, width, stride, want_slots=False)
    assert got[0] == 0 and (got[1] == np.uint64(SENTINEL)).all()
    same(got[2:], want[1:])
    # Width 0 with Slots: refused here (mv has results); the exact width works
    assert read_device(ctx, 0, stride)[0] == 0x04
    got = read_device(ctx, WIDEST_R, WIDEST_R)
    assert got[0] == 0 and np.array_equal(got[1], want[0][:, :WIDEST_R])


def aux_vec(funcs=("fib", "one"), types="sig"):
    sig = {"fib": [I32], "one": [], "xref": [EXTERNREF], "add": [I64, I64]}
    func_of = [None if i % 3 == 2 else i % 3 for i in range(N)]
    rows = [[((i * 7) % 15, I32)] if f == 0 else [] for i, f in enumerate(func_of)]
    return Vec(list(funcs), [sig[f] for f in funcs] if types == "sig" else types, func_of, rows)


@pytest.mark.gpu
def test_gpu_failures_leave_the_staging_runnable(built):
    """Every refused call leaves the context as it was: the staged vector still runs and gives
    what it gave before."""
    from wasmedge_amd import batch
    ctx = calls_ctx(N, wasm=AUX)
    try:
        vec = aux_vec()
        assert stage_device(ctx, vec) == 0, last_error(ctx)
        ctx.run()
        base = both_reads_agree(ctx, 1, "baseline")
        assert not base[2].any() and base[0].any() and set(int(x) for x in base[1]) == {0, 1}

        def still_runs(case):
            ctx.run()
            same(base, both_reads_agree(ctx, 1, case), case)

        fo = vec.fo()
        fo[90], fo[40] = 7, 2
        assert stage_device(ctx, vec, fo=fo) == 0x04 and b"FuncOf[40]" in last_error(ctx), last_error(ctx)
        still_runs("FuncOf out of range")
        assert stage_device(ctx, vec, null_fo=True) == 0x04
        still_runs("null FuncOf")
        assert stage_device(ctx, vec, stride=0) == 0x04
        still_runs("stride too small")
        assert stage_device(ctx, vec, null_slots=True) == 0x04
        still_runs("null slots")
        assert stage_device(ctx, vec, slots_off=4) == 0x04
        still_runs("misaligned slots")
        assert stage_device(ctx, vec, drop_lens=True) == 0x04
        still_runs("ParamLens without ParamTypes")
        assert stage_device(ctx, aux_vec(("fib", "one", "xref"))) == 0x02 and b"externref" in last_error(ctx)
        still_runs("externref export named")
        # a wrong ParamTypes row is no failure of the call: the instances naming it get 0x83
        assert stage_device(ctx, aux_vec(types=[[I64], []])) == 0
        ctx.run()
        got = both_reads_agree(ctx, 1, "wrong types")
        assert [int(s) for s in got[2]] == [0x83 if i % 3 == 0 else 0 for i in range(N)]
        # the import export named and not called: the run succeeds ...
        assert stage_device(ctx, aux_vec(("fib", "one", "add"))) == 0, last_error(ctx)
        still_runs("import named")
        # ... called by one instance: BatchRun refuses, as after set_calls
        called = aux_vec(("fib", "one", "add"))
        called.func_of[10], called.rows[10] = 2, [(1, I64), (2, I64)]
        assert stage_device(ctx, called) == 0, last_error(ctx)
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.run()
        assert e.value.code == 0x02
        stage_host(ctx, called)
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.run()
        assert e.value.code == 0x02
        assert stage_device(ctx, vec) == 0
        still_runs("after the import")
        # the uniform reader has no rows for a call vector, and this one none for a uniform run
        d = [Dev(np.full((N, 1), SENTINEL, np.uint64)), Dev(np.full(N, 0x77, np.uint8))]
        try:
            assert batch.lib().WasmEdge_BatchResultsDevice(ctx._h, d[0].ptr, 1, 1, d[1].ptr, None).Code == 0x04
            assert (d[0].numpy() == np.uint64(SENTINEL)).all() and (d[1].numpy() == 0x77).all()
        finally:
            for b in d:
                b.free()
        still_runs("BatchResultsDevice")
        ctx.set_args("one", np.zeros((N, 0), batch.VALUE_DTYPE))
        ctx.run()
        got = read_device(ctx, 1, 1)
        assert got[0] == 0x04 and b"BatchResultsDevice" in last_error(ctx) and untouched(got)
        # no completed run: after a Reset, as BatchResults
        assert stage_device(ctx, vec) == 0
        ctx.reset()
        got = read_device(ctx, 1, 1)
        assert got[0] == 0x04 and untouched(got)
        still_runs("after reset")
        # an externref result staged by the host path has no device rows
        xv = aux_vec(("fib", "one", "xref"))
        xv.func_of[1], xv.rows[1] = 2, [(5, EXTERNREF)]
        stage_host(ctx, xv)
        ctx.run()
        got = read_device(ctx, 1, 1)
        assert got[0] == 0x02 and b"externref" in last_error(ctx) and untouched(got)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_two_shards_refuse(built):
    """One device buffer cannot serve several devices: RuntimeError with a message, and the
    host path goes on working."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(SPIN, N, devices=[0, 0])
    try:
        vec = spin_vec()
        assert stage_device(ctx, vec) == 0x02 and b"multi-device" in last_error(ctx)
        stage_host(ctx, vec)
        ctx.run()
        got = read_device(ctx, 1, 1)
        assert got[0] == 0x02 and b"multi-device" in last_error(ctx) and untouched(got)
        want = read_host(ctx, 1)
        assert not want[2].any() and want[0].any()
    finally:
        ctx.close()


def spin_vec(flip_func=None, flip_arg=None):
    func_of = [None if i % 3 == 2 else i % 3 for i in range(N)]
    rows = [[(i * 20, I32)] if f == 0 else [((i * 7) % 15, I32)] if f == 1 else [] for i, f in enumerate(func_of)]
    if flip_func is not None:
        func_of[flip_func], rows[flip_func] = None, []
    if flip_arg is not None:
        rows[flip_arg] = [(rows[flip_arg][0][0] ^ 1, I32)]
    return Vec(["spin", "fib"], [[I32], [I32]], func_of, rows)


@pytest.mark.gpu
def test_gpu_resumable_slices_and_suspended_snapshots(built):
    """Between slices, after the resume that finishes, at once after a restore that permutes
    the instances across waves, and after the resume of that: CallsResultsDevice equals
    results() every time, and the sequence staged on the device equals the one staged through
    set_calls (the host copy of the vector is fetched for the snapshot, the device copy
    uploaded again after the mapped restore)."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(SPIN, N, device=0, max_steps=1500, resumable=True)
    perm = [(i * 37 + 11) % N for i in range(N)]
    assert sorted(perm) == list(range(N)) and any(p // 64 != i // 64 for i, p in enumerate(perm))
    vec = spin_vec()

    def sequence(stage):
        ctx.reset()
        stage()
        ctx.run()
        r = [both_reads_agree(ctx, 1, "first slice")]
        susp = r[0][2] == SUSPENDED
        assert susp.any() and not susp.all() and ctx.suspended() == int(susp.sum())
        assert not r[0][0][susp].any()
        snap = ctx.snapshot(invocation=True)
        try:
            ctx.resume(4000)
            r.append(both_reads_agree(ctx, 1, "second slice"))
            ctx.resume(0)
            r.append(both_reads_agree(ctx, 1, "finished"))
            assert not r[2][2].any() and ctx.suspended() == 0
            ctx.restore(snap, src_of=perm)
            r.append(both_reads_agree(ctx, 1, "restored"))
            same(r[3], [x[perm] for x in r[0]], "restored rows are the sources'")
            ctx.resume(0)
            r.append(both_reads_agree(ctx, 1, "restored and finished"))
            same(r[4], [x[perm] for x in r[2]], "finished rows are the sources'")
        finally:
            snap.close()
        return r

    try:
        def on_device():
            assert stage_device(ctx, vec) == 0, last_error(ctx)

        dev = sequence(on_device)
        host = sequence(lambda: stage_host(ctx, vec))
        for k, (a, b) in enumerate(zip(dev, host)):
            same(a, b, "step %d" % k)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [(256, 256), (64, 1024), (1024, 192)])
def test_gpu_fingerprint_through_the_restage_rule(built, monkeypatch, blocks):
    """A restored invocation runs again only under the vector it was captured with: one other
    FuncOf entry or one other argument wants a new staging (0x04), the same vector -- staged
    again, by a kernel of another block size -- does not. The fingerprint is a sum over table
    words and cells, so it must not depend on the launch geometry (WB_ARGS_BLOCK)."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(SPIN, N, device=0, resumable=True)
    try:
        a = spin_vec()
        monkeypatch.setenv("WB_ARGS_BLOCK", str(blocks[0]))
        assert stage_device(ctx, a) == 0, last_error(ctx)
        ctx.run()
        snap = ctx.snapshot(invocation=True)   # (before any read: it fetches the vector itself)
        try:
            first = both_reads_agree(ctx, 1, "first")
            monkeypatch.setenv("WB_ARGS_BLOCK", str(blocks[1]))
            for other in (spin_vec(flip_func=N - 1), spin_vec(flip_arg=N - 3)):
                assert stage_device(ctx, other) == 0
                ctx.restore(snap)
                with pytest.raises(batch.WasmEdgeError) as e:
                    ctx.run()
                assert e.value.code == 0x04
            assert stage_device(ctx, a) == 0
            ctx.restore(snap)
            ctx.run()
            same(first, both_reads_agree(ctx, 1, "restaged"))
        finally:
            snap.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_restage_compares_with_what_lies_staged(built):
    """The restage rule compares a restored invocation with the arguments that lie staged on the
    device, not with the invocation restored last: a second restore under another staging still
    wants a new one (0x04), and of two snapshots taken under two stagings and restored in turn
    a Run is possible after exactly the one whose arguments are staged. Host staging, so every
    CallsResultsDevice after a restore uploads the call vector again; it equals results()."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(SPIN, N, device=0, resumable=True)
    snaps = []
    try:
        vecs = spin_vec(), spin_vec(flip_func=N - 1, flip_arg=N - 3)
        want = []
        for k, vec in enumerate(vecs):
            stage_host(ctx, vec)
            ctx.run()
            want.append(both_reads_agree(ctx, 1, "run %d" % k))
            snaps.append(ctx.snapshot(invocation=True))
        assert not np.array_equal(want[0][1], want[1][1])   # (the flipped lane makes no call)
        for _ in range(2):   # the second vector is the staged one
            ctx.restore(snaps[0])
            same(want[0], both_reads_agree(ctx, 1, "first restored"))
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.run()
        assert e.value.code == 0x04
        ctx.restore(snaps[1])
        same(want[1], both_reads_agree(ctx, 1, "second restored"))
        ctx.run()
        same(want[1], both_reads_agree(ctx, 1, "second run again"))
        ctx.restore(snaps[0])
        stage_host(ctx, vecs[0])
        ctx.run()
        same(want[0], both_reads_agree(ctx, 1, "first staged and run again"))
    finally:
        for s in snaps:
            s.close()
        ctx.close()


@pytest.fixture(scope="module")
def tensor_child(built):
    """tests/calls_tensor_child.py, once: the torch mirror in a process where torch initialises
    its device before the first context exists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "calls_tensor_child.py")],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
def test_gpu_tensor_mirror(tensor_child):
    """set_calls_tensor / calls_results_tensor on the mixed vector equal the host path, result
    counts, statuses and instruction counts included; a non-contiguous, a CPU and a
    wrong-dtype tensor each raise ValueError."""
    res = tensor_child
    assert res["values_equal"] and res["lens_equal"] and res["status_equal"] and res["counts_equal"], res
    assert res["padding_kept"] and res["allocated_equal"] and res["memories_equal"], res
    assert res["refused"] == {"non_contiguous": True, "cpu": True, "dtype": True, "func_of_dtype": True,
                              "out_non_contiguous": True, "out_cpu": True, "lens_dtype": True}, res
