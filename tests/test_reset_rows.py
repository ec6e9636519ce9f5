"""Reset rewrites a wave's rows below its write mark with stores issued back to back
(batch_kernel.hip reset_rows / reset_state): in the interpreter launch (the deferred Reset,
fused_reset) and in wb_mem_init_kernel's write-mark path (WB_FUSED_RESET=0, a timed Reset, a
host accessor before the run, every granule above 4 bytes).

The helper writes rows in chunks of 8 (RR_CHUNK), the rest of a range as 4, 2 and 1 rows;
the data segments of 0, 1, 5, 8, 9, 17, 64 and 65 words sit around those sizes, and the
per-lane write marks put the end of the zero rows at every remainder.

Expected values come from the oracle (a fresh Instance's invoke, memory and memory hash) and
from a fresh context that only made the last call; the default path and WB_FUSED_RESET=0
must agree bit for bit.
"""
import os
import sys

import numpy as np
import pytest

from wasmedge_amd.wat import assemble

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

I32 = 0x7F
PAGE = 65536
DWORDS = [0, 1, 5, 8, 9, 17, 64, 65]
NS = [1, 64, 65]
PATTERNS = ["none", "low", "mixed"]

# poke(addr, val): stores val at addr (a lane with val 0 stores nothing), bumps the global,
# returns the word at addr; peek(addr) stores nothing: the word at addr + 0x10001 * global.
# drop / init: the passive segment (LS_DROPPED): init traps once drop ran
WAT = r"""
(module
  (memory (export "memory") 1)
  (global $g (mut i32) (i32.const 7))
  %s
  (data $p "\a1\b2\c3\d4")
  (func (export "poke") (param $a i32) (param $v i32) (result i32)
    (if (local.get $v) (then (i32.store (local.get $a) (local.get $v))))
    (global.set $g (i32.add (global.get $g) (i32.const 1)))
    (i32.load (local.get $a)))
  (func (export "peek") (param $a i32) (result i32)
    (i32.add (i32.load (local.get $a)) (i32.mul (global.get $g) (i32.const 0x10001))))
  (func (export "drop") (param $a i32) (param $v i32) (result i32)
    (data.drop $p)
    (i32.store (local.get $a) (local.get $v))
    (global.get $g))
  (func (export "init") (param $a i32) (result i32)
    (memory.init $p (local.get $a) (i32.const 0) (i32.const 4))
    (i32.add (i32.load (local.get $a)) (global.get $g))))
"""


def image(d):
    """the data segment's bytes: d words, none of them zero"""
    return np.array([(0x9E3779B1 * (k + 1)) | 0x01000001 for k in range(d)], np.uint64).astype("<u4").tobytes()


def wasm(d):
    seg = "" if d == 0 else '(data (i32.const 0) "%s")' % "".join("\\%02x" % b for b in image(d))
    return assemble(WAT % seg)


def addresses(pattern, n, d):
    """(addr, val) of each lane's poke; val 0: the lane stores nothing (write mark 0)"""
    rows = []
    for i in range(n):
        k = i % 5
        if pattern == "none" or (pattern == "mixed" and k == 0):
            rows.append([4 * (i % 7), 0])                        # no store
        elif pattern == "low":
            rows.append([4 * d + 20 + 4 * (i % 9), 0xA5000001 + i])   # just above the image, every remainder
        elif k == 1:
            rows.append([0, 0xB0000001 + i])                     # below / at the start of the image
        elif k == 2:
            rows.append([4 * max(d - 1, 0), 0xC0000001 + i])     # the image's last word
        elif k == 3:
            rows.append([4 * d + 4 * i, 0xD0000001 + i])         # above the image
        else:
            rows.append([4 * (d + 37 + 3 * i) + 1, 0xE0000001 + i])   # further up, unaligned
    if pattern == "mixed" and n > 1:
        rows[n - 1] = [PAGE - 4, 0xF00DF00D]                     # the page's last word: every row
    return rows


class Expected:
    """The oracle's answer to `func(addr)` on a fresh instance, per distinct address."""

    def __init__(self, wasm_bytes, func, addrs, cost_limit=0):
        import oracle_py as O
        m = O.Module(wasm_bytes)
        self.by_addr = {}
        for a in sorted(set(addrs)):
            inst = O.Instance(m, cost_limit=cost_limit)
            code, vals, cnt, mh = inst.invoke(func, [a])
            self.by_addr[a] = (code, vals[0] & 0xFFFFFFFF if vals else None, cnt, mh,
                               inst.memory(0, PAGE), inst.cost_sum())
        self.addrs = addrs

    def check(self, got, what):
        vals, st, cnt, mh, mem, costs = got
        for i, a in enumerate(self.addrs):
            code, val, ocnt, omh, omem, ocost = self.by_addr[a]
            assert int(st[i]) == code, (what, i)
            if code == 0:
                assert int(vals[i]) == val, (what, i)
            assert int(cnt[i]) == ocnt, (what, i)
            assert int(mh[i]) == omh, (what, i)
            assert mem[i].tobytes() == omem, (what, i)
            if costs is not None:
                assert int(costs[i]) == ocost, (what, i)


def call(ctx, func, rows):
    from wasmedge_amd import batch
    rets, st, cnt = ctx.execute(func, batch.make_values(rows, [I32] * len(rows[0])), 1)
    return np.array([int(x[0]) & 0xFFFFFFFF for x in batch.ret_ints(rets)], np.uint64), st.copy(), cnt.copy()


def observe(ctx, func, addrs, costs=False):
    """the last call and everything a host can see after it"""
    vals, st, cnt = call(ctx, func, [[a] for a in addrs])
    mh = ctx.memory_hash().copy()
    mem, mst = ctx.read_memories(PAGE)
    assert not mst.any()
    return vals, st, cnt, mh, mem.copy(), ctx.total_costs().copy() if costs else None


def same(a, b, what):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y), what


def sequences(ctx, dirty, pokes, last, addrs, costs=False):
    """every Reset sequence on one context, each from a dirtied state; yields (name, observed)"""
    def soil():
        call(ctx, dirty, pokes)
    soil()
    ctx.reset(timed=False)                       # deferred to the launch
    yield "poke,reset,peek", observe(ctx, last, addrs, costs)
    soil()
    ctx.reset(timed=False)
    ctx.reset(timed=False)
    yield "reset,reset,peek", observe(ctx, last, addrs, costs)
    soil()
    ctx.reset(timed=True)                        # the memory kernel, at once
    ctx.reset(timed=False)
    yield "timed reset,reset,peek", observe(ctx, last, addrs, costs)
    soil()
    ctx.reset(timed=False)
    ctx.memory_hash()                            # a host accessor settles the Reset first
    yield "reset,hash,peek", observe(ctx, last, addrs, costs)
    soil()
    ctx.reset(timed=False)
    ctx.read_memories(64)
    yield "reset,read,peek", observe(ctx, last, addrs, costs)


def run_case(monkeypatch, d, n, patterns, dirty="poke", last="peek", **kw):
    """The sequences for each pattern, on one context per Reset path (their memories stay
    dirty from one pattern to the next) against a fresh context and the oracle per pattern."""
    from wasmedge_amd import batch
    if isinstance(patterns, str):
        patterns = [patterns]
    w = wasm(d)
    costs = "cost_limit" in kw
    monkeypatch.delenv("WB_FUSED_RESET", raising=False)
    ctxs = {}
    try:
        for mode in ("default", "0"):
            ctxs[mode] = batch.BatchContext(w, n, device=0, **kw)
            if "memory_granule" in kw:
                assert ctxs[mode].memory_granule() == kw["memory_granule"]
        for pattern in patterns:
            pokes = addresses(pattern, n, d)
            addrs = [r[0] for r in pokes]
            exp = Expected(w, last, addrs, cost_limit=kw.get("cost_limit", 0))
            fresh_ctx = batch.BatchContext(w, n, device=0, **kw)
            try:
                fresh = observe(fresh_ctx, last, addrs, costs)
            finally:
                fresh_ctx.close()
            exp.check(fresh, "fresh")
            seen = {}
            for mode in ("default", "0"):
                # (read at every Reset)
                if mode == "0":
                    monkeypatch.setenv("WB_FUSED_RESET", "0")
                else:
                    monkeypatch.delenv("WB_FUSED_RESET", raising=False)
                for name, got in sequences(ctxs[mode], dirty, pokes, last, addrs, costs):
                    what = (d, n, pattern, mode, name)
                    exp.check(got, what)
                    same(got, fresh, what)
                    seen[(mode, name)] = got
            for (mode, name), got in seen.items():
                if mode == "0":
                    same(got, seen[("default", name)], (d, n, pattern, name, "default against WB_FUSED_RESET=0"))
    finally:
        for c in ctxs.values():
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DWORDS)
def test_reset_rows(monkeypatch, d, n):
    """Every write-mark pattern and Reset sequence for a data segment of d words on n lanes."""
    run_case(monkeypatch, d, n, PATTERNS)


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [16, 128])
def test_reset_rows_granules(monkeypatch, granule):
    """wb_mem_init_kernel's write-mark path with g > 0: rows rounded up to granules, image
    words that differ by lane."""
    for d in (9, 65):
        run_case(monkeypatch, d, 65, "mixed", memory_granule=granule)
    run_case(monkeypatch, 5, 64, "low", memory_granule=granule)


@pytest.mark.gpu
def test_reset_rows_cost_limit(monkeypatch):
    """With metering the Reset restores the gas total too (LS_COST, both words)."""
    run_case(monkeypatch, 9, 65, "mixed", cost_limit=1 << 40)
    run_case(monkeypatch, 17, 64, "low", cost_limit=1 << 40)


@pytest.mark.gpu
def test_reset_rows_dropped_segment(monkeypatch):
    """A dropped passive segment is back after the Reset (LS_DROPPED): memory.init from it
    works again, as on a fresh instance."""
    run_case(monkeypatch, 9, 65, "low", dirty="drop", last="init")
    run_case(monkeypatch, 0, 64, "low", dirty="drop", last="init")


def test_addresses_cover_the_marks():
    """(no GPU) the patterns give marks of 0, below, inside and above the image, every
    remainder of the chunk size above it, and the page's last word."""
    for d in DWORDS:
        low = addresses("low", 65, d)
        assert {(r[0] // 4 + 1 - d) % 8 for r in low} == set(range(8))
        mixed = addresses("mixed", 65, d)
        marks = [0 if r[1] == 0 else r[0] + 4 for r in mixed]
        assert 0 in marks and PAGE in marks
        assert any(0 < m <= 4 * d for m in marks) == (d > 0)
        assert any(m > 4 * d for m in marks)
        assert all(r[1] == 0 for r in addresses("none", 65, d))
        assert len(image(d)) == 4 * d and all(np.frombuffer(image(d), "<u4"))
