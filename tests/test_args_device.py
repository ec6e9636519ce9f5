"""Device-resident arguments and results: WasmEdge_BatchSetArgsDevice stages a run from rows
of 64-bit slots in device memory and WasmEdge_BatchResultsDevice writes its results, statuses
and counts into device memory (include/wasmedge_batch.h; Python: set_args_tensor /
results_tensor, slots_of).

The yardstick is always the host path (set_args / results) on the same context and module,
which other tests pin to the oracle: device and host must agree bit for bit. Device buffers
come from the HIP runtime the library is bound to (hipMalloc and friends through the
library's own handle), so nothing here needs torch; the tensor mirror runs once in a process
of its own (tests/args_tensor_child.py). 130 instances: two full waves and two lanes.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from wasmedge_amd.wat import assemble

I32, I64, F32, F64, V128, FUNCREF, EXTERNREF = 0x7F, 0x7E, 0x7D, 0x7C, 0x7B, 0x70, 0x6F
N = 130
ONES = 0xFFFFFFFF00000000
SENTINEL = 0x5AA55AA55AA55AA5
UNREACHABLE, SUSPENDED = 0x89, 0x07

# mix folds every parameter into every result, so a cell taken from the wrong slot or half
# changes an output; trap_odd executes unreachable for an odd argument; spin is a counted loop
WAT = r"""
(module
  (func (export "mix") (param $a i32) (param $b i64) (param $c f32) (param $d v128) (param $e f64) (param $f i32)
        (result i32 i64 v128 f64)
    (local $h i64)
    (local.set $h
      (i64.add (i64.mul (i64.extend_i32_u (local.get $a)) (i64.const 0x9E3779B97F4A7C15))
      (i64.add (i64.mul (local.get $b) (i64.const 0xC2B2AE3D27D4EB4F))
      (i64.add (i64.mul (i64.extend_i32_u (i32.reinterpret_f32 (local.get $c))) (i64.const 0x165667B19E3779F9))
      (i64.add (i64.mul (i64x2.extract_lane 0 (local.get $d)) (i64.const 0x27D4EB2F165667C5))
      (i64.add (i64.mul (i64x2.extract_lane 1 (local.get $d)) (i64.const 0x85EBCA77C2B2AE63))
      (i64.add (i64.mul (i64.reinterpret_f64 (local.get $e)) (i64.const 0xFF51AFD7ED558CCD))
               (i64.mul (i64.extend_i32_u (local.get $f)) (i64.const 0xC4CEB9FE1A85EC53)))))))))
    (i32.wrap_i64 (i64.shr_u (local.get $h) (i64.const 29)))
    (i64.rotl (local.get $h) (i64.const 17))
    (v128.xor (local.get $d) (i64x2.replace_lane 1 (i64x2.splat (local.get $h)) (i64.mul (local.get $h) (i64.const 3))))
    (f64.reinterpret_i64 (i64.xor (local.get $h) (i64.reinterpret_f64 (local.get $e)))))
  (func (export "id32") (param $x i32) (result i32) (local.get $x))
  (func (export "nop"))
  (func (export "fref") (param $r funcref) (result funcref) (local.get $r))
  (func (export "xref") (param $r externref) (result externref) (local.get $r))
  (func (export "trap_odd") (param $x i32) (result i64)
    (if (i32.and (local.get $x) (i32.const 1)) (then (unreachable)))
    (i64.mul (i64.extend_i32_u (local.get $x)) (i64.const 0x100000001)))
  (func (export "spin") (param $n i32) (result i32)
    (local $i i32) (local $s i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $n)))
      (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (local.get $i)))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.get $s)))
"""
MIX_P, MIX_R = [I32, I64, F32, V128, F64, I32], [I32, I64, V128, F64]
SIGS = {"mix": (MIX_P, MIX_R), "id32": ([I32], [I32]), "nop": ([], []), "fref": ([FUNCREF], [FUNCREF]),
        "xref": ([EXTERNREF], [EXTERNREF]), "trap_odd": ([I32], [I64]), "spin": ([I32], [I32])}


def wasm():
    return assemble(WAT)


def slots_of(types):
    return sum(2 if t == V128 else 1 for t in types)


class Dev:
    """A device array behind ctypes: hipMalloc / hipMemcpy / hipFree looked up through the
    library's own handle, whose search covers its dependencies -- the HIP runtime the library
    is bound to answers."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            from wasmedge_amd import batch
            batch.lib()
            cls._hip = ctypes.CDLL(batch.LIB_PATH)
            cls._hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            cls._hip.hipFree.argtypes = [ctypes.c_void_p]
            cls._hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        return cls._hip

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype, self.nbytes = arr.shape, arr.dtype, arr.nbytes
        self.ptr = ctypes.c_void_p()
        assert self.hip().hipMalloc(ctypes.byref(self.ptr), max(arr.nbytes, 8)) == 0
        if arr.nbytes:
            assert self.hip().hipMemcpy(self.ptr, arr.ctypes.data, arr.nbytes, 1) == 0   # host to device

    def numpy(self):
        out = np.zeros(self.shape, self.dtype)
        if self.nbytes:
            assert self.hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0   # device to host
        return out

    def free(self):
        self.hip().hipFree(self.ptr)


def last_error(ctx):
    from wasmedge_amd import batch
    return batch.lib().WasmEdge_BatchGetLastError(ctx._h)


def stage_device(ctx, func, slots, types=None, length=None, stride=None, null=False):
    """WasmEdge_BatchSetArgsDevice on a [n][stride] uint64 array (uploaded here); its code"""
    from wasmedge_amd import batch
    types = SIGS[func][0] if types is None else types
    length = len(types) if length is None else length
    tarr = np.array(types, np.uint32)
    dev = Dev(slots)
    try:
        name = func.encode()
        return batch.lib().WasmEdge_BatchSetArgsDevice(
            ctx._h, batch._String(len(name), name), tarr.ctypes.data if len(types) else None, length,
            None if null else dev.ptr, slots.shape[1] if stride is None else stride).Code
    finally:
        dev.free()


def stage_host(ctx, func, slots):
    """The same arguments through set_args: value k of a row from its slot (two for a v128);
    make_values keeps the low 32 bits of an i32 / f32 / funcref, as SetArgs reads them."""
    from wasmedge_amd import batch
    types = SIGS[func][0]
    rows = []
    for r in slots:
        row, at = [], 0
        for t in types:
            row.append(int(r[at]) | (int(r[at + 1]) << 64) if t == V128 else int(r[at]))
            at += 2 if t == V128 else 1
        rows.append(row)
    ctx.set_args(func, batch.make_values(rows, types) if types else np.zeros((ctx.n, 0), batch.VALUE_DTYPE))


def read_host(ctx, func, retlen=None):
    """results() as the rows ResultsDevice has to write: (slots [n][slots of the first
    retlen results], status, counts)"""
    types = SIGS[func][1]
    retlen = len(types) if retlen is None else min(retlen, len(types))
    rets, st, cnt = ctx.results(len(types))
    cols = []
    for k, t in enumerate(types[:retlen]):
        cols.append(rets["lo"][:, k])
        if t == V128:
            cols.append(rets["hi"][:, k])
        else:
            assert not rets["hi"][:, k].any()
    out = np.stack(cols, axis=1).astype(np.uint64) if cols else np.zeros((ctx.n, 0), np.uint64)
    return out, st.copy(), cnt.copy()


def read_device(ctx, retlen, stride, fill=SENTINEL, want_slots=True):
    """WasmEdge_BatchResultsDevice into sentinel-filled device arrays: (code, slots [n][stride],
    status, counts)"""
    from wasmedge_amd import batch
    d_slots = Dev(np.full((ctx.n, stride), fill, np.uint64))
    d_st = Dev(np.full(ctx.n, 0x77, np.uint8))
    d_cnt = Dev(np.full(ctx.n, fill, np.uint64))
    try:
        code = batch.lib().WasmEdge_BatchResultsDevice(ctx._h, d_slots.ptr if want_slots else None, retlen, stride,
                                                       d_st.ptr, d_cnt.ptr).Code
        return code, d_slots.numpy(), d_st.numpy(), d_cnt.numpy()
    finally:
        for d in (d_slots, d_st, d_cnt):
            d.free()


def mix_slots(n, seed):
    """Random rows for mix: every bit pattern, NaN payloads in the f32 and f64 slots of some
    rows, and all-ones upper halves on the i32 and f32 slots (they must be ignored)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 64, (n, slots_of(MIX_P)), dtype=np.uint64)
    for col in (0, 2, 6):   # a, c, f
        s[:, col] = (s[:, col] & np.uint64(0xFFFFFFFF)) | np.uint64(ONES)
    s[::3, 2] = (s[::3, 2] & np.uint64(0x007FFFFF)) | np.uint64(0x7F800001 | ONES)    # f32 NaNs
    s[1::3, 5] = (s[1::3, 5] & np.uint64((1 << 52) - 1)) | np.uint64(0xFFF0000000000001)   # f64 NaNs
    return s


def both_reads_agree(ctx, func, case):
    """ResultsDevice (every result, rows two slots wider than they need to be) against
    results(); returns the host triple"""
    want, st, cnt = read_host(ctx, func)
    width = want.shape[1]
    code, got, dst, dcnt = read_device(ctx, len(SIGS[func][1]), width + 2)
    assert code == 0, (case, last_error(ctx))
    assert np.array_equal(got[:, :width], want), case
    assert (got[:, width:] == np.uint64(SENTINEL)).all(), case
    assert np.array_equal(dst, st) and np.array_equal(dcnt, cnt), case
    return want, st, cnt


@pytest.fixture(scope="module")
def ctx130(built):
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, device=0)
    yield ctx
    ctx.close()


# ---- no GPU needed ------------------------------------------------------------------------

def test_symbols_refuse_a_null_context(built):
    from wasmedge_amd import batch
    L = batch.lib()
    types = np.array([I32], np.uint32)
    assert L.WasmEdge_BatchSetArgsDevice(None, batch._String(1, b"f"), types.ctypes.data, 1, None, 1).Code == 0x04
    assert L.WasmEdge_BatchResultsDevice(None, None, 1, 1, None, None).Code == 0x04


def test_slots_of():
    from wasmedge_amd import batch
    for t in (I32, I64, F32, F64, FUNCREF, EXTERNREF):
        assert batch.slots_of([t]) == 1
    assert batch.slots_of([V128]) == 2
    assert batch.slots_of([]) == 0
    assert batch.slots_of(MIX_P) == 7 and batch.slots_of(MIX_R) == 5
    assert batch.slots_of((V128, I32, V128)) == 5
    with pytest.raises(ValueError):
        batch.slots_of([I32, 0x40])


def test_tensor_arguments_are_checked_before_any_call():
    """What is no contiguous device tensor of the right dtype and shape is refused with
    ValueError before the library is called (the context here has no handle at all)."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext.__new__(batch.BatchContext)
    ctx.n, ctx._h = 4, None
    rows = np.zeros((4, 2), np.int64)
    with pytest.raises(ValueError):
        ctx.set_args_tensor("f", [I64, I64], rows)   # not a tensor
    with pytest.raises(ValueError):
        ctx.set_args_tensor("f", [I64], None)        # a row needs slots
    with pytest.raises(ValueError):
        ctx.set_args_tensor("f", [0x12], rows)       # not a value type
    with pytest.raises(ValueError):
        ctx.results_tensor(1, out=rows)
    with pytest.raises(ValueError):
        ctx.results_tensor(1, status=np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        ctx.results_tensor(1, counts=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        ctx.results_tensor(-1, out=rows)
    with pytest.raises(ValueError):
        ctx.results_tensor([I32, 0x12], out=rows)


# ---- GPU ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 130])
def test_gpu_mix_all_four_paths(built, ctx130, n):
    """Host or device staging, host or device results: the four combinations give the same
    values, statuses and counts."""
    from wasmedge_amd import batch
    ctx = ctx130 if n == N else batch.BatchContext(wasm(), n, device=0)
    try:
        slots = mix_slots(n, 7 + n)
        stage_host(ctx, "mix", slots)
        ctx.run()
        host = both_reads_agree(ctx, "mix", "host staging")
        assert not host[1].any() and host[0].any()
        ctx.reset()
        # rows three slots wider than a row of mix, the padding all ones
        wide = np.full((n, slots.shape[1] + 3), 0xFFFFFFFFFFFFFFFF, np.uint64)
        wide[:, :slots.shape[1]] = slots
        assert stage_device(ctx, "mix", wide) == 0, last_error(ctx)
        ctx.run()
        dev = both_reads_agree(ctx, "mix", "device staging")
        for a, b in zip(host, dev):
            assert np.array_equal(a, b)
    finally:
        if ctx is not ctx130:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("retlen", [0, 2, 4, 6])
def test_gpu_stride_and_return_len(built, ctx130, retlen):
    """A row receives the first min(ReturnLen, 4) results of mix; its other slots and the
    padding up to Stride keep the sentinel."""
    ctx = ctx130
    assert stage_device(ctx, "mix", mix_slots(N, 21)) == 0, last_error(ctx)
    ctx.run()
    want, st, cnt = read_host(ctx, "mix", retlen)
    width = want.shape[1]
    assert width == [0, 2, 5, 5][retlen // 2]
    stride = slots_of(MIX_R) + 4
    code, got, dst, dcnt = read_device(ctx, retlen, stride)
    assert code == 0, last_error(ctx)
    assert np.array_equal(got[:, :width], want)
    assert (got[:, width:] == np.uint64(SENTINEL)).all()
    assert np.array_equal(dst, st) and np.array_equal(dcnt, cnt)
    # NULL Slots: the status and count arrays alone
    code, got, dst, dcnt = read_device(ctx, retlen, stride, want_slots=False)
    assert code == 0 and (got == np.uint64(SENTINEL)).all()
    assert np.array_equal(dst, st) and np.array_equal(dcnt, cnt)


@pytest.mark.gpu
def test_gpu_trapped_rows_read_zero(built, ctx130):
    ctx = ctx130
    slots = (np.arange(N, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(N)) & np.uint64(0xFFFFFFFF)
    slots = slots.reshape(N, 1) | np.uint64(ONES)
    odd = (slots[:, 0] & np.uint64(1)).astype(bool)
    assert odd.any() and not odd.all()
    stage_host(ctx, "trap_odd", slots)
    ctx.run()
    host = read_host(ctx, "trap_odd")
    assert stage_device(ctx, "trap_odd", slots) == 0, last_error(ctx)
    ctx.run()
    want, st, cnt = both_reads_agree(ctx, "trap_odd", "trap_odd")
    for a, b in zip(host, (want, st, cnt)):
        assert np.array_equal(a, b)
    assert [int(s) for s in st] == [UNREACHABLE if o else 0 for o in odd]
    assert not want[odd].any() and want[~odd].all()


@pytest.mark.gpu
def test_gpu_no_parameters_and_funcrefs(built, ctx130):
    """nop stages with NULL Slots and has no rows to read; a null funcref is 0xFFFFFFFF in the
    slot's low half, a function index its own value, the upper half zero on the way out."""
    ctx = ctx130
    assert stage_device(ctx, "nop", np.zeros((N, 0), np.uint64), null=True, stride=0) == 0, last_error(ctx)
    ctx.run()
    code, got, st, cnt = read_device(ctx, 3, 2)
    assert code == 0 and (got == np.uint64(SENTINEL)).all() and not st.any()
    host = read_host(ctx, "nop")
    assert np.array_equal(cnt, host[2])
    refs = np.array([0xFFFFFFFF if i % 3 == 0 else i % 7 for i in range(N)], np.uint64).reshape(N, 1)
    assert stage_device(ctx, "fref", refs | np.uint64(ONES)) == 0, last_error(ctx)
    ctx.run()
    want, st, _ = both_reads_agree(ctx, "fref", "fref")
    assert not st.any() and np.array_equal(want, refs)
    stage_host(ctx, "fref", refs)
    ctx.run()
    assert np.array_equal(both_reads_agree(ctx, "fref", "fref, host staging")[0], refs)


@pytest.mark.gpu
def test_gpu_errors_leave_the_staging_runnable(built, ctx130):
    """Every refused call leaves the context as it was: the staged id32 still runs and gives
    what it gave before."""
    from wasmedge_amd import batch
    ctx = ctx130
    args = (np.arange(N, dtype=np.uint64) * np.uint64(40503) + np.uint64(9)).reshape(N, 1)
    assert stage_device(ctx, "id32", args) == 0, last_error(ctx)
    ctx.run()
    base = both_reads_agree(ctx, "id32", "baseline")
    assert np.array_equal(base[0], args & np.uint64(0xFFFFFFFF))

    def still_runs(case):
        ctx.run()
        for a, b in zip(base, both_reads_agree(ctx, "id32", case)):
            assert np.array_equal(a, b), case

    two = np.zeros((N, 2), np.uint64)
    assert stage_device(ctx, "id32", args, types=[I64]) == 0x83
    still_runs("wrong type")
    assert stage_device(ctx, "id32", two, types=[I32, I32]) == 0x83
    still_runs("wrong length")
    assert stage_device(ctx, "mix", mix_slots(N, 1), types=MIX_P[:-1] + [I64]) == 0x83
    still_runs("wrong last type")
    assert stage_device(ctx, "nosuch", args, types=[I32]) == 0x05
    still_runs("unknown name")
    assert stage_device(ctx, "mix", mix_slots(N, 1), stride=slots_of(MIX_P) - 1) == 0x04
    still_runs("stride too small")
    assert stage_device(ctx, "id32", args, null=True) == 0x04
    still_runs("null slots")
    assert stage_device(ctx, "xref", args) == 0x02 and b"externref" in last_error(ctx)
    still_runs("externref")
    code, got, st, cnt = read_device(ctx, 1, 0)
    assert code == 0x04 and (got == np.uint64(SENTINEL)).all() and (st == 0x77).all() \
        and (cnt == np.uint64(SENTINEL)).all()
    still_runs("results: stride too small")
    # an externref result staged by the host path has no device rows either
    ctx.set_args("xref", batch.make_values([[i] for i in range(N)], [EXTERNREF]))
    ctx.run()
    code, got, st, cnt = read_device(ctx, 1, 1)
    assert code == 0x02 and b"externref" in last_error(ctx) and (got == np.uint64(SENTINEL)).all()
    assert stage_device(ctx, "id32", args) == 0
    still_runs("after xref")
    # per-instance calls have no device rows
    ctx.set_calls(["id32"], [0] * N, [[(i, I32)] for i in range(N)])
    ctx.run()
    assert read_device(ctx, 1, 1)[0] == 0x04 and last_error(ctx)
    rets, st, _ = ctx.results(1)
    assert not st.any() and [int(x) for x in rets["lo"][:, 0]] == list(range(N))
    # no completed run: after a Reset, as BatchResults
    assert stage_device(ctx, "id32", args) == 0
    ctx.reset()
    code, got, st, cnt = read_device(ctx, 1, 1)
    assert code == 0x04 and (got == np.uint64(SENTINEL)).all() and (st == 0x77).all()
    still_runs("after reset")


@pytest.mark.gpu
def test_gpu_two_shards_refuse(built):
    """One device buffer cannot serve several devices: RuntimeError with a message, and the
    host path goes on working."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, devices=[0, 0])
    try:
        args = np.arange(N, dtype=np.uint64).reshape(N, 1)
        assert stage_device(ctx, "id32", args) == 0x02 and b"multi-device" in last_error(ctx)
        stage_host(ctx, "id32", args)
        ctx.run()
        code, got, st, cnt = read_device(ctx, 1, 1)
        assert code == 0x02 and b"multi-device" in last_error(ctx)
        assert (got == np.uint64(SENTINEL)).all() and (st == 0x77).all()
        assert np.array_equal(read_host(ctx, "id32")[0], args)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_resumable_slices(built):
    """Between slices suspended rows read zero with 0x07, as results() has them; after the
    resume that finishes them every row holds its value."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, device=0, max_steps=1500, resumable=True)
    try:
        trips = (np.arange(N, dtype=np.uint64) * np.uint64(20)).reshape(N, 1)
        assert stage_device(ctx, "spin", trips | np.uint64(ONES)) == 0, last_error(ctx)
        ctx.run()
        want, st, _ = both_reads_agree(ctx, "spin", "first slice")
        susp = st == SUSPENDED
        assert susp.any() and not susp.all() and ctx.suspended() == int(susp.sum())
        assert not want[susp].any() and not st[~susp].any()
        ctx.resume(3000)
        _, st2, _ = both_reads_agree(ctx, "spin", "second slice")
        assert int((st2 == SUSPENDED).sum()) == ctx.suspended() <= int(susp.sum())
        ctx.resume(0)
        dev = both_reads_agree(ctx, "spin", "finished")
        assert not dev[1].any() and ctx.suspended() == 0
        stage_host(ctx, "spin", trips)
        ctx.run()
        ctx.resume(0)
        for a, b in zip(dev, both_reads_agree(ctx, "spin", "host staging")):
            assert np.array_equal(a, b)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [(256, 256), (64, 1024), (1024, 192)])
def test_gpu_fingerprint_through_the_restage_rule(built, monkeypatch, blocks):
    """A restored invocation runs again only under the arguments it was captured with: other
    device arguments want a new staging (0x04), the same ones -- staged again, by kernels of
    another block size -- do not. The fingerprint is a sum over cells, so it must not depend on
    the launch geometry (WB_ARGS_BLOCK)."""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, device=0, resumable=True)
    try:
        a = mix_slots(N, 31)
        b = a.copy()
        b[N - 1, 4] ^= np.uint64(1 << 40)   # one bit of one cell of the last row
        stage_host(ctx, "mix", a)
        ctx.run()
        host = read_host(ctx, "mix")
        monkeypatch.setenv("WB_ARGS_BLOCK", str(blocks[0]))
        assert stage_device(ctx, "mix", a) == 0, last_error(ctx)
        ctx.run()
        snap = ctx.snapshot(invocation=True)
        try:
            monkeypatch.setenv("WB_ARGS_BLOCK", str(blocks[1]))
            assert stage_device(ctx, "mix", b) == 0
            ctx.restore(snap)
            with pytest.raises(batch.WasmEdgeError) as e:
                ctx.run()
            assert e.value.code == 0x04
            assert stage_device(ctx, "mix", a) == 0
            ctx.restore(snap)
            ctx.run()
            for x, y in zip(host, both_reads_agree(ctx, "mix", "restaged")):
                assert np.array_equal(x, y)
        finally:
            snap.close()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def tensor_child(built):
    """tests/args_tensor_child.py, once: the torch mirror in a process where torch initialises
    its device before the first context exists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "args_tensor_child.py")],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
def test_gpu_tensor_mirror(tensor_child):
    """set_args_tensor / results_tensor on mix equal the host path, statuses and counts
    included; a non-contiguous, a CPU and a wrong-dtype tensor each raise ValueError."""
    res = tensor_child
    assert res["values_equal"] and res["status_equal"] and res["counts_equal"], res
    assert res["padding_kept"] and res["allocated_equal"], res
    assert res["refused"] == {"non_contiguous": True, "cpu": True, "dtype": True,
                              "out_non_contiguous": True, "out_cpu": True, "out_dtype": True}, res
