"""Device-resident spans: WasmEdge_BatchWriteMemoriesSpansDevice / ReadMemoriesSpansDevice take
every instance's own offset and length from 64-bit slots in device memory (a column of a
BatchResultsDevice buffer as it lies), write the status bytes to device memory and report the
number of instances out of bounds (include/wasmedge_batch.h; Python:
write_memories_spans_tensor / read_memories_spans_tensor / last_spans_tiled_waves).

Expected values come from numpy images of the memories and from the existing host variants
(write_memories / read_memories), never from the new calls. 130 instances: two full waves and
a partial one of two lanes. Device buffers come from the HIP runtime the library is bound to
(test_memio.DeviceRows), so nothing here needs torch; the tensor mirror runs once in a process
of its own (tests/memspans_tensor_child.py).
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from wasmedge_amd.wat import assemble

import test_memio as M
from test_memio import DeviceRows, GRANULES, N, OOB, np_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wasmedge_amd", "csrc")
PAGE = 65536
SPANS = ["WasmEdge_BatchWriteMemoriesSpansDevice", "WasmEdge_BatchReadMemoriesSpansDevice"]
JUNK = np.uint64(0xDEADBEEF) << np.uint64(32)

# obs(x): fills [ptr, ptr + len) with the bytes x, x + 1, ... and returns (ptr, len), both
# computed from x -- an allocator's answer that differs from instance to instance
OBS_WAT = r"""
(module
  (memory (export "memory") 1)
  (func (export "obs") (param $x i32) (result i32 i32)
    (local $p i32) (local $n i32) (local $i i32)
    (local.set $p (i32.add (i32.const 4096) (i32.mul (local.get $x) (i32.const 24))))
    (local.set $n (i32.add (i32.const 16) (i32.mul (local.get $x) (i32.const 5))))
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $n)))
      (i32.store8 (i32.add (local.get $p) (local.get $i)) (i32.add (local.get $x) (local.get $i)))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.get $p) (local.get $n)))
"""

HEADER_MAIN = r"""
#include "wasmedge_batch.h"
uint32_t caller(WasmEdge_BatchContext *c, const uint64_t *slots, uint8_t *rows, uint8_t *st) {
  uint32_t oob = 0;
  WasmEdge_Result r = WasmEdge_BatchWriteMemoriesSpansDevice(c, slots, 2, 16, slots + 1, 2, 64, rows, 64, st, &oob);
  if (r.Code) return r.Code;
  r = WasmEdge_BatchReadMemoriesSpansDevice(c, slots, 2, 16, 0, 0, 64, rows, 64, 0, &oob);
  return r.Code + oob + WasmEdge_BatchGetLastSpansTiledWaves(c);
}
"""


# ---- without a GPU ------------------------------------------------------------------------
def test_header_compiles_as_c(tmp_path):
    """The header with a caller of the three new functions, as C."""
    src = tmp_path / "caller.c"
    src.write_text(HEADER_MAIN)
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "caller.o")])


def test_spans_symbols_refuse_null_arguments(built):
    """A NULL context gives WrongVMWorkflow from both entry points, and the report 0."""
    from wasmedge_amd import batch
    L = batch.lib()
    oob = ctypes.c_uint32(7)
    for name in SPANS:
        assert getattr(L, name)(None, None, 0, 0, None, 0, 8, None, 8, None, None).Code == 0x04, name
        assert getattr(L, name)(None, None, 1, 0, None, 1, 0, None, 0, None, ctypes.addressof(oob)).Code == 0x04, name
    assert oob.value == 7
    assert L.WasmEdge_BatchGetLastSpansTiledWaves(None) == 0


def test_spans_tensor_refuses_before_the_library(built):
    """A non-tensor, a wrong dtype, shape, device or stride: ValueError from a context that has
    no handle, so no library call can have happened."""
    import torch
    from wasmedge_amd import batch
    ctx = batch.BatchContext.__new__(batch.BatchContext)
    ctx.n = N
    ctx._h = None
    rows = torch.zeros((N, 16), dtype=torch.uint8)   # (not on the device)
    for fn in (ctx.write_memories_spans_tensor, ctx.read_memories_spans_tensor):
        for bad in (np.zeros((N, 16), np.uint8), rows, torch.zeros((N, 16), dtype=torch.int8),
                    torch.zeros(N * 16, dtype=torch.uint8), torch.zeros((N - 1, 16), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                fn(bad)
    # the span and status checks, on a stand-in that passes for rows on a device

    class Rows(torch.Tensor):
        is_cuda = True
    fake = torch.zeros((N, 16), dtype=torch.uint8).as_subclass(Rows)
    good = torch.zeros(N, dtype=torch.int64)
    for bad in ([0] * N, np.zeros(N, np.int64), torch.zeros(N, dtype=torch.int32), torch.zeros(N - 1, dtype=torch.int64),
                torch.zeros((N, 1), dtype=torch.int64), torch.zeros(N, dtype=torch.int64, device="meta"),
                torch.zeros(1, dtype=torch.int64).expand(N)):   # (the last: element stride 0)
        with pytest.raises(ValueError):
            ctx.write_memories_spans_tensor(fake, offsets=bad)
        with pytest.raises(ValueError):
            ctx.read_memories_spans_tensor(fake, offsets=good, lens=bad)
    for bad in (np.zeros(N, np.uint8), torch.zeros(N, dtype=torch.int8), torch.zeros(N + 1, dtype=torch.uint8),
                torch.zeros((N, 2), dtype=torch.uint8)[:, 0], torch.zeros(N, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError):
            ctx.write_memories_spans_tensor(fake, status=bad)
    for kw in ({"length": 17}, {"length": -1}, {"offset": -1}, {"offset": 1 << 32}):
        with pytest.raises(ValueError):
            ctx.read_memories_spans_tensor(fake, **kw)


def test_rehearsal_under_sanitizers(tmp_path):
    """tests/c/memspans_rehearsal.cpp: the plan and move bodies as host code under the address
    and undefined-behaviour sanitizers, a thread per GPU thread, against a byte model -- the
    GPU cases below at granules 4, 8, 16 and 128. No report, no differing byte."""
    exe = str(tmp_path / "rehearsal")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-pthread", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "memspans_rehearsal.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)   # (it stays under a minute)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ---- GPU cases ----------------------------------------------------------------------------
def dev_of(arr):
    """any [n, ...] array as device bytes"""
    arr = np.ascontiguousarray(arr)
    return DeviceRows(arr.view(np.uint8).reshape(arr.shape[0], -1))


class Spans:
    """Offsets and lengths as columns of one [N][width] uint64 device buffer, junk in every
    upper half and in the slots between."""

    def __init__(self, own=None, lens=None, width=3, junk=JUNK):
        slots = np.full((N, width), 0xFEEDFACECAFEF00D, np.uint64)
        self.off_col = self.len_col = None
        if own is not None:
            slots[:, 1] = np.asarray(own, np.uint64) | junk
            self.off_col = 1
        if lens is not None:
            slots[:, width - 1] = np.asarray(lens, np.uint64) | junk
            self.len_col = width - 1
        self.width = width
        self.dev = dev_of(slots)

    def args(self):
        """(OffsetSlots, OffsetStride, LenSlots, LenStride)"""
        base = self.dev.ptr.value
        return (base + 8 * self.off_col if self.off_col is not None else None,
                self.width if self.off_col is not None else 0,
                base + 8 * self.len_col if self.len_col is not None else None,
                self.width if self.len_col is not None else 0)

    def free(self):
        self.dev.free()


def spans_call(ctx, name, rows_dev, span_args, offset, length, status=True, stride=None):
    """one spans call on a DeviceRows: (call-level code, status bytes or None, out of bounds)"""
    from wasmedge_amd import batch
    st = dev_of(np.full(N, 0x77, np.uint8)) if status else None
    oob = ctypes.c_uint32(0xFFFF)
    po, so, pl, sl = span_args
    try:
        r = getattr(batch.lib(), name)(ctx._h, po, so, offset, pl, sl, length, rows_dev.ptr if rows_dev else None,
                                       rows_dev.shape[1] if stride is None else stride,
                                       st.ptr if st else None, ctypes.addressof(oob))
        return r.Code, (st.numpy().reshape(N) if st else None), oob.value
    finally:
        if st:
            st.free()


def sizes_of(ctx):
    return np.array([ctx.memory_pages(i) for i in range(N)], np.int64) * PAGE


def images_of(ctx, sizes):
    """every instance's whole memory through the host variant, [N][max size] (zero past a
    smaller instance's size)"""
    image, st = ctx.read_memories(int(sizes.max()), lens=sizes.astype(np.uint32))
    assert not st.any()
    return image


def round_trip(ctx, rng, offset, length, own=None, lens=None, stride=None, tiled=None, status=True, sums=False):
    """Write rows through the spans call, compare every memory with the numpy image, read them
    back through the spans call into 0x77-filled rows; status bytes, the out-of-bounds count and
    the tiled waves on both. Returns the instances in bounds."""
    from wasmedge_amd import batch
    stride = length if stride is None else stride
    sizes = sizes_of(ctx)
    image = images_of(ctx, sizes)
    start = offset + (np.asarray(own, np.int64) if own is not None else np.zeros(N, np.int64))
    ln = np.asarray(lens, np.int64) if lens is not None else np.full(N, length, np.int64)
    fits = start + ln <= sizes
    want_st = np.where(fits, 0, OOB).astype(np.uint8)
    rows = rng.integers(1, 256, (N, stride), dtype=np.uint8)
    sp = Spans(own, lens)
    src, dst = DeviceRows(rows), DeviceRows(np.full((N, stride), 0x77, np.uint8))
    try:
        code, st, oob = spans_call(ctx, SPANS[0], src, sp.args(), offset, length, status)
        assert code == 0, batch.lib().WasmEdge_BatchGetLastError(ctx._h)
        assert oob == int((~fits).sum())
        assert st is None or np.array_equal(st, want_st)
        if tiled is not None:
            assert ctx.last_spans_tiled_waves() == tiled
        assert np.array_equal(src.numpy(), rows)
        for i in range(N):
            if fits[i]:
                image[i, start[i]:start[i] + ln[i]] = rows[i, :ln[i]]
        assert np.array_equal(images_of(ctx, sizes), image)
        code, st, oob = spans_call(ctx, SPANS[1], dst, sp.args(), offset, length, status)
        assert code == 0 and oob == int((~fits).sum())
        assert st is None or np.array_equal(st, want_st)
        if tiled is not None:
            assert ctx.last_spans_tiled_waves() == tiled
        want = np.full((N, stride), 0x77, np.uint8)
        for i in range(N):
            if fits[i]:
                want[i, :ln[i]] = rows[i, :ln[i]]
        assert np.array_equal(dst.numpy(), want)
        assert np.array_equal(images_of(ctx, sizes), image)
        if sums:   # the module's own view of what it was given
            assert fits.all() and (ln == length).all() and stride == length
            got = M.run(ctx, "sum", [[int(start[i]), length] for i in range(N)], 1)
            assert got == [int(x) for x in np_sum(rows)]
    finally:
        for d in (src, dst):
            d.free()
        sp.free()
    return fits


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_uniform_aligned(built, granule):
    """Every instance's own offset 1024, Offset 256, 4096 bytes: all three waves tile, and the
    image is exact."""
    ctx = M.context(granule)
    try:
        round_trip(ctx, np.random.default_rng(granule), 256, 4096, own=[1024] * N, tiled=3, sums=True)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_mixed_waves(built, granule):
    """Wave 0 uniform at 512, wave 1 scattered, the partial wave uniform at 8: two waves tile,
    one goes lane by lane."""
    own = [512 if i < 64 else (i * 37) % 509 if i < 128 else 8 for i in range(N)]
    ctx = M.context(granule)
    try:
        round_trip(ctx, np.random.default_rng(10 + granule), 0, 1000, own=own, tiled=2, sums=True)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_uniform_unaligned(built, granule):
    """One start for everybody, 3 past a word: no wave tiles, the bytes are still exact."""
    ctx = M.context(granule)
    try:
        round_trip(ctx, np.random.default_rng(20 + granule), 3, 1000, own=[1024] * N, tiled=0, sums=True)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_lengths(built, granule):
    """Len 67, len_i = i % 68, zeros included: tails merge byte by byte, on the tiled path
    (rows 68 apart) and on the per-lane path (rows 67 apart), and a read leaves the bytes of a
    row past len_i as they were."""
    lens = [i % 68 for i in range(N)]
    ctx = M.context(granule)
    try:
        rng = np.random.default_rng(30 + granule)
        round_trip(ctx, rng, 2048, 67, lens=lens, stride=68, tiled=3)
        round_trip(ctx, rng, 0, 67, own=[4096] * N, lens=lens, stride=67, tiled=0)
        round_trip(ctx, rng, 5, 67, own=[(i * 37) % 509 for i in range(N)], lens=lens, stride=72, tiled=0)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_out_of_bounds_inside_a_uniform_wave(built, granule, monkeypatch):
    """Instances of 1, 2 and 3 pages and one start near a page's end: exactly numpy's set gets
    0x88 and keeps memory and row, the count is numpy's, with and without PerInstance; the
    class is decided over the instances that move, so every wave still tiles."""
    monkeypatch.setenv("WB_RELAYOUT", "0")
    ctx = M.context(granule, limits="1 4")
    try:
        assert M.run(ctx, "grow", [[i % 3] for i in range(N)], 1) == [1] * N
        rng = np.random.default_rng(40 + granule)
        for own, length in ((PAGE - 128, 4096), (2 * PAGE - 64, 256)):
            for status in (True, False):
                fits = round_trip(ctx, rng, 0, length, own=[own] * N, tiled=3, status=status)
                assert 0 < int(fits.sum()) < N
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_reserved_pool_boundary(built, granule, monkeypatch):
    """One reserved page, two more from pool rows: a uniform range across either page edge
    tiles, crosses into the pool rows and is exact."""
    monkeypatch.setenv("WB_RELAYOUT", "0")
    ctx = M.context(granule, memory_reserve_pages=1)
    try:
        assert M.run(ctx, "grow", [[2]] * N, 1) == [1] * N
        assert ctx.reserved_pages() == 1
        rng = np.random.default_rng(50 + granule)
        for own in (PAGE - 128, 2 * PAGE - 64):
            fits = round_trip(ctx, rng, 0, 4096, own=[own] * N, tiled=3, sums=True)
            assert fits.all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_slot_form(built):
    """Offsets as column 1 of an [N][3] uint64 buffer: 0xDEADBEEF in the upper halves changes
    nothing against clean slots."""
    own = [(i * 37) % 509 for i in range(N)]
    rows = np.random.default_rng(60).integers(1, 256, (N, 200), dtype=np.uint8)
    images = []
    for junk in (JUNK, np.uint64(0)):
        ctx = M.context(16)
        sp, src = Spans(own, junk=junk), DeviceRows(rows)
        try:
            code, st, oob = spans_call(ctx, SPANS[0], src, sp.args(), 100, 200)
            assert code == 0 and oob == 0 and not st.any()
            images.append(ctx.read_memories(PAGE)[0])
        finally:
            src.free()
            sp.free()
            ctx.close()
    want = np.zeros((N, PAGE), np.uint8)
    for i in range(N):
        want[i, 100 + own[i]:300 + own[i]] = rows[i]
    assert np.array_equal(images[0], want) and np.array_equal(images[1], want)


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [4, 128])
def test_gpu_end_to_end(built, granule):
    """obs(x) returns (ptr, len) computed from x; BatchRun, BatchResultsDevice into a device
    buffer, its two columns with stride 2 to the spans read: no host copy in between, and every
    row is what the instance wrote at the pointer it returned."""
    from wasmedge_amd import batch
    xs = [i % 7 for i in range(N)]
    ctx = batch.BatchContext(assemble(OBS_WAT), N, device=0, memory_granule=granule)
    res = dev_of(np.full((N, 2), 0x5555555555555555, np.uint64))
    rst, cnt = dev_of(np.full(N, 0x77, np.uint8)), dev_of(np.zeros(N, np.uint64))
    dst = DeviceRows(np.full((N, 48), 0x77, np.uint8))
    try:
        ctx.set_args("obs", batch.make_values([[x] for x in xs], [M.I32]))
        ctx.run()
        assert batch.lib().WasmEdge_BatchResultsDevice(ctx._h, res.ptr, 2, 2, rst.ptr, cnt.ptr).Code == 0
        base = res.ptr.value
        code, st, oob = spans_call(ctx, SPANS[1], dst, (base, 2, base + 8, 2), 0, 48)
        assert code == 0 and oob == 0 and not st.any()
        want = np.full((N, 48), 0x77, np.uint8)
        for i, x in enumerate(xs):
            want[i, :16 + 5 * x] = (x + np.arange(16 + 5 * x)) & 0xFF
        assert np.array_equal(dst.numpy(), want)
        slots = res.numpy().view(np.uint64)
        assert [int(v) for v in slots[:, 0]] == [4096 + 24 * x for x in xs]
    finally:
        for d in (res, rst, cnt, dst):
            d.free()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_write_mark(built, granule):
    """A spans write raises the write mark: after reset(), peek reads the initial image."""
    ctx = M.context(granule, limits="2 4")
    sp, src = Spans([100000 + 4 * (i % 3) for i in range(N)]), DeviceRows(np.full((N, 64), 0xEE, np.uint8))
    try:
        code, st, oob = spans_call(ctx, SPANS[0], src, sp.args(), 0, 64)
        assert code == 0 and oob == 0 and not st.any()
        assert M.run(ctx, "peek", [[100008]] * N, 1) == [0xEEEEEEEE] * N
        ctx.reset()
        assert M.run(ctx, "peek", [[100008]] * N, 1) == [0] * N
        assert M.run(ctx, "peek", [[100064]] * N, 1) == [0] * N
        # ... and a write directly after a Reset that did not wait lands after the init kernels
        M.run(ctx, "fill", [[7, 100000, 64]] * N, 0)
        ctx.reset(timed=False)
        code, st, oob = spans_call(ctx, SPANS[0], src, sp.args(), 64, 64)
        assert code == 0 and oob == 0
        assert M.run(ctx, "peek", [[100000]] * N, 1) == [0] * N
        assert M.run(ctx, "peek", [[100072]] * N, 1) == [0xEEEEEEEE] * N
    finally:
        src.free()
        sp.free()
        ctx.close()


@pytest.mark.gpu
def test_gpu_call_level_failures(built):
    """Every refused call leaves memory (read through the host variant), the rows and a
    0x77-filled status buffer as they were, and sets a message."""
    from wasmedge_amd import batch
    L = batch.lib()
    ctx = M.context(16)
    rows = np.random.default_rng(70).integers(1, 256, (N, 16), dtype=np.uint8)
    assert not ctx.write_memories(rows, offset=64).any()
    before = ctx.read_memories(PAGE)[0]
    fresh = np.full((N, 16), 0x33, np.uint8)
    lens = np.full(N, 8, np.uint64)
    lens[77] = lens[5] = 9
    long_sp, good_sp = Spans([64] * N, lens), Spans([64] * N, [8] * N)
    short = dev_of(np.zeros(N - 1, np.uint64))   # N - 1 slots from the library's own hipMalloc
    po, so, pl, sl = good_sp.args()

    def refused(name, args, offset, length, want, stride=None, word=None):
        dev = DeviceRows(fresh)
        try:
            code, st, oob = spans_call(ctx, name, dev, args, offset, length, stride=stride)
            assert code == want, (name, code)
            msg = L.WasmEdge_BatchGetLastError(ctx._h)
            assert msg and (word is None or word in msg), msg
            assert oob == 0xFFFF and bytes(st) == b"\x77" * N
            assert np.array_equal(dev.numpy(), fresh)
            assert np.array_equal(ctx.read_memories(PAGE)[0], before)
        finally:
            dev.free()
    try:
        for name in SPANS:
            refused(name, long_sp.args(), 0, 8, 0x04, word=b"instance 5")
            refused(name, (po + 4, so, pl, sl), 0, 8, 0x04)
            refused(name, (po, so, pl + 4, sl), 0, 8, 0x04)
            refused(name, (po, 0, pl, sl), 0, 8, 0x04)
            refused(name, (po, so, pl, 0), 0, 8, 0x04)
            refused(name, good_sp.args(), 0, 16, 0x04, stride=15)
            refused(name, (short.ptr.value, 1, None, 0), 0, 8, 0x02)
            refused(name, (None, 0, short.ptr.value, 1), 0, 8, 0x02)
            assert getattr(L, name)(ctx._h, po, so, 0, pl, sl, 8, None, 16, None, None).Code == 0x04
        # (the good spans are good: the same call goes through)
        dev = DeviceRows(fresh)
        try:
            code, st, oob = spans_call(ctx, SPANS[1], dev, good_sp.args(), 0, 8)
            assert code == 0 and oob == 0 and np.array_equal(dev.numpy()[:, :8], rows[:, :8])
        finally:
            dev.free()
    finally:
        ctx.close()
    dev = DeviceRows(fresh)
    try:
        ctx = batch.BatchContext(M.wasm(), N, memory_granule=16, devices=[0, 0])
        try:
            for name in SPANS:
                assert spans_call(ctx, name, dev, good_sp.args(), 0, 8)[0] == 0x02, name
                assert b"device" in L.WasmEdge_BatchGetLastError(ctx._h)
        finally:
            ctx.close()
        ctx = batch.BatchContext(assemble(M.NOMEM_WAT), N, device=0)
        try:
            for name in SPANS:
                assert spans_call(ctx, name, dev, good_sp.args(), 0, 8)[0] == OOB, name
        finally:
            ctx.close()
        assert np.array_equal(dev.numpy(), fresh)
    finally:
        for d in (dev, short):
            d.free()
        long_sp.free()
        good_sp.free()


@pytest.fixture(scope="module")
def tensor_child(built):
    """tests/memspans_tensor_child.py, once: the torch tensor variants in a process where torch
    initialises its device before the first context exists."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "memspans_tensor_child.py")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_gpu_tensor_variants(tensor_child, granule):
    """results_tensor columns as offsets / lens and a status tensor: the rows, the status bytes
    and the count equal the host variant's for the same spans."""
    res = tensor_child[str(granule)]
    assert len(res) == 2
    for r in res:
        assert r["read_equals_host"] and r["write_equals_host"] and r["status_equals_host"] \
            and r["count_equals_host"] and r["tiled_waves"] == r["tiled_expected"], r
