"""Bulk linear-memory transfer: WasmEdge_BatchWriteMemories / ReadMemories and their Device
variants move a [NumInstances][Stride] array into or out of every instance's memory in one
call (the batched WasmEdge_MemoryInstanceSetData / GetData, wasmedge.h:2552-2569).

Expected values come from the oracle (an Instance's invoke + memory, hash_bytes) and from
numpy, never from the code under test. 130 instances: three waves, the last one partial.
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

from wasmedge_amd.wat import assemble

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

I32 = 0x7F
N = 130
GRANULES = [4, 8, 16, 128]
OOB = 0x88

# grow(k); fill(seed, off, len): a xorshift byte stream through i32.store8; sum(off, len):
# the sum of byte * (index + 1) mod 2^32; peek(a): the word at a
WAT = r"""
(module
  (memory (export "memory") %s)
  (func (export "grow") (param $k i32) (result i32) (memory.grow (local.get $k)))
  (func (export "fill") (param $x i32) (param $off i32) (param $len i32)
    (local $i i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $len)))
      (local.set $x (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 13))))
      (local.set $x (i32.xor (local.get $x) (i32.shr_u (local.get $x) (i32.const 17))))
      (local.set $x (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 5))))
      (i32.store8 (i32.add (local.get $off) (local.get $i)) (local.get $x))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l))))
  (func (export "sum") (param $off i32) (param $len i32) (result i32)
    (local $i i32) (local $s i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $len)))
      (local.set $s (i32.add (local.get $s)
        (i32.mul (i32.load8_u (i32.add (local.get $off) (local.get $i)))
                 (i32.add (local.get $i) (i32.const 1)))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.get $s))
  (func (export "peek") (param $a i32) (result i32) (i32.load (local.get $a))))
"""
NOMEM_WAT = r"""(module (func (export "f") (result i32) (i32.const 1)))"""

BULK = ["WasmEdge_BatchWriteMemories", "WasmEdge_BatchReadMemories",
        "WasmEdge_BatchWriteMemoriesDevice", "WasmEdge_BatchReadMemoriesDevice"]


def wasm(limits="1 4"):
    return assemble(WAT % limits)


def np_sum(rows):
    """sum(off, len) of each row, as the module computes it"""
    w = np.arange(1, rows.shape[1] + 1, dtype=np.uint64)
    return (rows.astype(np.uint64) * w).sum(axis=1) & np.uint64(0xFFFFFFFF)


def run(ctx, func, rows, nret):
    from wasmedge_amd import batch
    rets, st, _ = ctx.execute(func, batch.make_values(rows, [I32] * len(rows[0])), nret)
    assert not st.any(), (func, st)
    return [int(x[0]) for x in batch.ret_ints(rets)] if nret else None


def context(granule, n=N, limits="1 4", **kw):
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(limits), n, device=0, memory_granule=granule, **kw)
    assert ctx.memory_granule() == granule
    return ctx


class DeviceRows:
    """A [n][stride] byte buffer in device memory from the HIP runtime the library itself
    is bound to, for the Device variants: hipMalloc and friends are looked up through the
    library's own handle, whose search covers its dependencies, so whichever libamdhip64
    the loader gave it (a process may have mapped more than one) is the one that answers."""
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

    def __init__(self, rows):
        self.shape = rows.shape
        self.ptr = ctypes.c_void_p()
        assert self.hip().hipMalloc(ctypes.byref(self.ptr), max(rows.size, 1)) == 0
        rows = np.ascontiguousarray(rows)
        assert self.hip().hipMemcpy(self.ptr, rows.ctypes.data, rows.size, 1) == 0   # host to device

    def numpy(self):
        out = np.zeros(self.shape, np.uint8)
        assert self.hip().hipMemcpy(out.ctypes.data, self.ptr, out.size, 2) == 0   # device to host
        return out

    def free(self):
        self.hip().hipFree(self.ptr)


def device_io(ctx, name, dev, offset=0, offsets=None, lens=None, length=None):
    """WasmEdge_Batch{Write,Read}MemoriesDevice on a DeviceRows; (call-level code, status)"""
    from wasmedge_amd import batch
    st = np.full(ctx.n, 0x77, np.uint8)
    r = getattr(batch.lib(), name)(ctx._h, offsets.ctypes.data if offsets is not None else None, offset,
                                   lens.ctypes.data if lens is not None else None,
                                   dev.shape[1] if length is None else length, dev.ptr, dev.shape[1],
                                   st.ctypes.data)
    return r.Code, st


def test_bulk_symbols_refuse_a_null_context(built):
    """The four entry points exist and give WrongVMWorkflow for a NULL context."""
    from wasmedge_amd import batch
    L = batch.lib()
    buf = ctypes.create_string_buffer(8)
    for name in BULK:
        r = getattr(L, name)(None, None, 0, None, 8, buf, 8, None)
        assert r.Code == 0x04, name


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_write_then_run(built, granule):
    """Rows written in one call are what the module then reads (sum), what the memory hash
    covers and what the per-instance host path returns."""
    import oracle_py as O
    rng = np.random.default_rng(granule)
    ctx = context(granule)
    try:
        for off, length in ((512, 4096), (516, 1000)):   # 16-byte and 4-byte aligned rows
            rows = rng.integers(0, 256, (N, length), dtype=np.uint8)
            ctx.reset()
            st = ctx.write_memories(rows, offset=off)
            assert not st.any()
            got = run(ctx, "sum", [[off, length]] * N, 1)
            assert got == [int(x) for x in np_sum(rows)]
            h = ctx.memory_hash()
            image = np.zeros(65536, np.uint8)
            for i in range(N):
                image[off:off + length] = rows[i]
                assert int(h[i]) == O.hash_bytes(image.tobytes(), 1), i
            for i in (0, 63, 64, 129):
                assert ctx.memory(i, off, length) == rows[i].tobytes(), i
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_run_then_read(built, granule):
    """What every instance wrote itself (fill, its own seed) comes back in one call, equal to
    the oracle instance's memory."""
    import oracle_py as O
    off, length = 33, 3000
    seeds = [(i * 2654435761 + 12345) & 0xFFFFFFFF or 1 for i in range(N)]
    ctx = context(granule)
    try:
        run(ctx, "fill", [[s, off, length] for s in seeds], 0)
        got, st = ctx.read_memories(4096)
        assert not st.any()
        m = O.Module(wasm())
        for i in range(N):
            inst = O.Instance(m)
            assert inst.invoke("fill", [seeds[i], off, length])[0] == 0
            assert got[i].tobytes() == inst.memory(0, 4096), i
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_shapes_round_trip(built, granule):
    """Lengths and offsets around every word, granule and page edge, uniform and per
    instance (mixed alignments, lengths 0..Len), rows 3 bytes wider than Len: each write
    reads back bit-exactly and changes nothing outside its ranges -- a numpy image of all
    memories follows every write and is compared with a read of both pages."""
    rng = np.random.default_rng(100 + granule)
    ctx = context(granule)
    try:
        assert run(ctx, "grow", [[1]] * N, 1) == [1] * N
        size = 2 * 65536
        image, st = ctx.read_memories(size)
        assert not st.any() and not image.any()
        for length in (0, 1, 3, 4, 5, 67, 4099):
            for offset in (0, 1, 2, 3, 125, 65536 - 5):
                for per_instance in (False, True):
                    offs = np.array([(i * 37) % 509 for i in range(N)], np.uint32) if per_instance else None
                    lens = np.array([i % (length + 1) for i in range(N)], np.uint32) if per_instance else None
                    rows = rng.integers(0, 256, (N, length + 3), dtype=np.uint8)
                    case = (length, offset, per_instance)
                    st = ctx.write_memories(rows, offset=offset, offsets=offs, lens=lens, length=length)
                    assert not st.any(), case
                    for i in range(N):
                        a = offset + (int(offs[i]) if per_instance else 0)
                        k = int(lens[i]) if per_instance else length
                        image[i, a:a + k] = rows[i, :k]
                    # the ranges read back; the row's other bytes stay as they were
                    out = np.full((N, length + 3), 0xA5, np.uint8)
                    _, st = ctx.read_memories(length, offset=offset, offsets=offs, lens=lens, out=out)
                    assert not st.any(), case
                    want = np.full((N, length + 3), 0xA5, np.uint8)
                    for i in range(N):
                        k = int(lens[i]) if per_instance else length
                        want[i, :k] = rows[i, :k]
                    assert np.array_equal(out, want), case
                    full, st = ctx.read_memories(size)
                    assert not st.any() and np.array_equal(full, image), case
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_pool_pages_and_bounds(built, granule, monkeypatch):
    """One reserved page, instances of 1, 2 and 3 pages (the pages past the first in pool
    rows): a range across a page edge lands in the instances that have the page; the others
    get 0x88 and keep their memory and their row."""
    monkeypatch.setenv("WB_RELAYOUT", "0")
    rng = np.random.default_rng(200 + granule)
    ctx = context(granule, memory_reserve_pages=1)
    try:
        assert run(ctx, "grow", [[i % 3] for i in range(N)], 1) == [1] * N
        assert ctx.reserved_pages() == 1
        pages = np.array([1 + i % 3 for i in range(N)])
        for edge in (65536, 131072):
            off = edge - 5
            before = ctx.memory_hash()
            rows = rng.integers(1, 256, (N, 10), dtype=np.uint8)
            st = ctx.write_memories(rows, offset=off)
            fits = pages * 65536 >= off + 10
            assert [int(s) for s in st] == [0 if f else OOB for f in fits], edge
            after = ctx.memory_hash()
            assert all(int(after[i]) == int(before[i]) for i in range(N) if not fits[i])
            out = np.full((N, 10), 0x5A, np.uint8)
            _, st = ctx.read_memories(10, offset=off, out=out)
            assert [int(s) for s in st] == [0 if f else OOB for f in fits], edge
            for i in range(N):
                assert out[i].tobytes() == (rows[i].tobytes() if fits[i] else b"\x5a" * 10), (edge, i)
            # the module sees the bytes (only the instances that have the page may look)
            from wasmedge_amd import batch
            rets, rst, _ = ctx.execute("sum", batch.make_values([[off, 10]] * N, [I32, I32]), 1)
            ints = batch.ret_ints(rets)
            want = np_sum(rows)
            for i in range(N):
                assert int(rst[i]) == (0 if fits[i] else OOB), (edge, i)
                if fits[i]:
                    assert int(ints[i][0]) == int(want[i]), (edge, i)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_reset_restores_bulk_writes(built, granule):
    """A bulk write raises the write mark, so Reset restores the bytes; and a write directly
    after a Reset that did not wait lands after the init kernels."""
    import oracle_py as O
    ctx = context(granule, limits="2 4")
    try:
        fresh = O.hash_bytes(bytes(131072), 2)
        assert all(int(h) == fresh for h in ctx.memory_hash())
        rows = np.full((N, 64), 0xEE, np.uint8)
        assert not ctx.write_memories(rows, offset=100000).any()
        assert all(int(h) != fresh for h in ctx.memory_hash())
        ctx.reset()
        assert all(int(h) == fresh for h in ctx.memory_hash())
        # dirty the memory from the module's side, reset without waiting, write at once
        run(ctx, "fill", [[7, 4096, 64]] * N, 0)
        ctx.reset(timed=False)
        st = ctx.write_memories([(0x01020300 + i).to_bytes(4, "little") for i in range(N)], offset=4100)
        assert not st.any()
        assert run(ctx, "peek", [[4100]] * N, 1) == [0x01020300 + i for i in range(N)]
        assert run(ctx, "peek", [[4096]] * N, 1) == [0] * N
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("partition", [0, 1])
def test_gpu_shards(built, partition):
    """Two shards on one device: Offsets, Lens and the rows are sliced by the placement and
    the status bytes gathered, with the single-device context's results; the device variants
    refuse (RuntimeError): one device buffer cannot serve several devices."""
    from wasmedge_amd import batch
    rng = np.random.default_rng(300 + partition)
    rows = rng.integers(0, 256, (N, 96), dtype=np.uint8)
    offs = np.array([(i * 37) % 509 for i in range(N)], np.uint32)
    lens = np.array([i % 97 for i in range(N)], np.uint32)
    # the last instances' ranges end past the first page: 0x88, in instance order
    offs[-3:] = 65536 - 40
    lens[-3:] = 96
    results = []
    for kw in ({}, {"devices": [0, 0], "partition": partition}):
        ctx = batch.BatchContext(wasm(), N, memory_granule=16, **({"device": 0} if not kw else kw))
        try:
            st = ctx.write_memories(rows, offset=1000, offsets=offs, lens=lens)
            rets, rst, _ = ctx.execute("sum", batch.make_values(
                [[1000 + int(offs[i]), int(lens[i])] for i in range(N)], [I32, I32]), 1)
            out = np.full((N, 100), 0x33, np.uint8)
            _, st2 = ctx.read_memories(96, offset=1000, offsets=offs, lens=lens, out=out)
            results.append((st, [int(x[0]) if rst[i] == 0 else None for i, x in enumerate(batch.ret_ints(rets))],
                            rst, out, st2, ctx.memory_hash()))
            if kw:
                dev = DeviceRows(rows)
                try:
                    for name in BULK[2:]:
                        assert device_io(ctx, name, dev)[0] == 0x02, name
                        assert b"device" in batch.lib().WasmEdge_BatchGetLastError(ctx._h)
                finally:
                    dev.free()
        finally:
            ctx.close()
    one, two = results
    assert [int(s) for s in one[0]] == [0] * (N - 3) + [OOB] * 3
    want = np.full((N, 100), 0x33, np.uint8)
    for i in range(N - 3):
        want[i, :lens[i]] = rows[i, :lens[i]]
    assert np.array_equal(one[3], want)
    sums = [int(np_sum(rows[i:i + 1, :lens[i]])[0]) if lens[i] else 0 for i in range(N)]
    assert one[1][:N - 3] == sums[:N - 3] and one[1][N - 3:] == [None] * 3
    assert one[1] == two[1]
    for k in (0, 2, 3, 4, 5):
        assert np.array_equal(one[k], two[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_device_variants(built, granule):
    """Rows in device memory go in and come out without crossing the host, with the host
    variants' results: 16-byte rows, 4-byte rows, per-instance offsets and lengths, and rows
    wider than Len; a device buffer too small for NumInstances rows is refused."""
    rng = np.random.default_rng(400 + granule)
    ctx = context(granule)
    try:
        for width, offset, per_instance in ((4096, 256, False), (68, 260, False), (67, 3, True)):
            offs = np.array([(i * 37) % 509 for i in range(N)], np.uint32) if per_instance else None
            lens = np.array([i % (width + 1) for i in range(N)], np.uint32) if per_instance else None
            rows = rng.integers(0, 256, (N, width + 4), dtype=np.uint8)
            ctx.reset()
            src = DeviceRows(rows)
            dst = DeviceRows(np.full((N, width + 4), 0xC3, np.uint8))
            try:
                code, st = device_io(ctx, BULK[2], src, offset, offs, lens, length=width)
                assert code == 0 and not st.any()
                host, st = ctx.read_memories(width, offset=offset, offsets=offs, lens=lens)
                assert not st.any()
                want = np.zeros((N, width), np.uint8)
                for i in range(N):
                    k = int(lens[i]) if per_instance else width
                    want[i, :k] = rows[i, :k]
                assert np.array_equal(host, want), (width, offset)
                code, st = device_io(ctx, BULK[3], dst, offset, offs, lens, length=width)
                assert code == 0 and not st.any()
                got = dst.numpy()
                for i in range(N):
                    k = int(lens[i]) if per_instance else width
                    assert got[i, :k].tobytes() == rows[i, :k].tobytes(), (width, offset, i)
                    assert got[i, k:].tobytes() == b"\xc3" * (width + 4 - k), (width, offset, i)
                assert np.array_equal(src.numpy(), rows)
                # NumInstances rows of this stride do not fit the allocation: refused, nothing moved
                if width == 4096:
                    small = DeviceRows(rows[:N // 2])
                    try:
                        for name in BULK[2:]:
                            assert device_io(ctx, name, small, offset, length=width)[0] == 0x02
                    finally:
                        small.free()
            finally:
                src.free()
                dst.free()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def tensor_child(built):
    """tests/memio_tensor_child.py, once: the torch tensor variants in a process where torch
    initialises its device before the first context exists."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "memio_tensor_child.py")],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_tensor_variants(tensor_child, granule):
    """A torch.uint8 tensor round-trips through write_memories_tensor / read_memories_tensor
    with the host variants' result, numpy's expectation and the module's own sum."""
    res = tensor_child[str(granule)]
    assert len(res) == 3
    for r in res:
        assert r["status_clear"] and r["host_equals_numpy"] and r["tensor_equals_host"] \
            and r["sum_equals_numpy"], r


@pytest.mark.gpu
def test_gpu_call_level_errors(built):
    """Stride < Len and a Lens[i] > Len fail the call with 0x04 and move nothing; a module
    without a memory gives 0x88."""
    from wasmedge_amd import batch
    L = batch.lib()
    ctx = context(16)
    try:
        before = ctx.memory_hash()
        buf = (ctypes.c_uint8 * (N * 16))(*([0xFF] * (N * 16)))
        st = (ctypes.c_uint8 * N)(*([0x77] * N))
        lens = (ctypes.c_uint32 * N)(*([8] * (N - 1) + [9]))
        for name in BULK[:2]:
            assert getattr(L, name)(ctx._h, None, 0, None, 16, buf, 15, st).Code == 0x04
            assert getattr(L, name)(ctx._h, None, 0, lens, 8, buf, 16, st).Code == 0x04
            assert getattr(L, name)(ctx._h, None, 0, None, 16, None, 16, st).Code == 0x04
        assert bytes(st) == b"\x77" * N and bytes(buf) == b"\xff" * (N * 16)
        assert np.array_equal(ctx.memory_hash(), before)
    finally:
        ctx.close()
    ctx = batch.BatchContext(assemble(NOMEM_WAT), N, device=0)
    try:
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.write_memories(np.zeros((N, 4), np.uint8))
        assert e.value.code == OOB
        with pytest.raises(batch.WasmEdgeError) as e:
            ctx.read_memories(4)
        assert e.value.code == OOB
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_bulk_write_beats_the_per_instance_loop(built):
    """64 bytes into each of 4,096 instances: one bulk call is at least 10x faster than the
    set_memory loop (which moves 512 KiB in four synchronous copies per instance), and
    leaves the same memory."""
    n = 4096
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    ctx = context(16, n=n)
    try:
        ctx.write_memories(rows, offset=1024)   # (the first launch loads the kernel)
        ctx.reset()
        t0 = time.perf_counter()
        st = ctx.write_memories(rows, offset=1024)
        t_bulk = time.perf_counter() - t0
        assert not st.any()
        h_bulk = ctx.memory_hash()
        ctx.reset()
        t0 = time.perf_counter()
        for i in range(n):
            ctx.set_memory(i, 1024, rows[i].tobytes())
        t_loop = time.perf_counter() - t0
        print("bulk write %.6f s, set_memory loop %.6f s, ratio %.1f" % (t_bulk, t_loop, t_loop / t_bulk))
        assert np.array_equal(ctx.memory_hash(), h_bulk)
        assert t_loop >= 10 * t_bulk
    finally:
        ctx.close()
