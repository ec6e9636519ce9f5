"""Instance snapshots: WasmEdge_BatchSnapshotCreate / Restore capture the state of every
instance between runs and restart instance i from the captured state of instance SrcOf[i].

Expected values come only from the oracle: one oracle_py.Instance per instance, invoked in
the same order; for a fork, instance i's twin runs init(seed[SrcOf[i]]) and then step(x[i]).
Every instance is compared, trapped ones included: status, returns, instruction counts,
memory hash, pages, globals, and the table through sum(). 130 instances: two waves and a
partial one.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from helpers import compare
from wasmedge_amd.wat import assemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = 0x7F
N = 130
GRANULES = [4, 8, 16, 128]

# init(seed): a xorshift stream of (seed * 53) % 1500 + 1 words from byte 4 * (seed % 7) (marks
# differ per lane and per wave, ranges cross 64-word tiles and every granule); seed % 5 == 0
# grows a page and stores into it; the globals, memory.init + data.drop, table slots.
# step(x): reads and mutates all of that; its call_indirect traps on a null slot after the
# mutations. scribble(): 8 pages, stores at both ends, the table grown far past its capacity.
# sum(): read-only checksum over memory, globals, table and page count. growsum(): grows a
# page and folds its words (zero in a fresh page).
WAT = r"""
(module
  (type $v (func (result i32)))
  (memory (export "memory") 1 8)
  (global $g (export "g") (mut i32) (i32.const 11))
  (global $h (export "h") (mut i64) (i64.const 22))
  (table $t (export "t") 4 funcref)
  (data $d "\01\02\03\04\05\06\07\08snapshot")
  (func $f0 (type $v) (i32.const 100))
  (func $f1 (type $v) (i32.const 201))
  (func $f2 (type $v) (i32.const 302))
  (elem (table $t) (i32.const 0) func $f0 $f0 $f0)
  (elem declare func $f1 $f2)
  (func $xs (param $x i32) (result i32)
    (local.set $x (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 13))))
    (local.set $x (i32.xor (local.get $x) (i32.shr_u (local.get $x) (i32.const 17))))
    (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 5))))
  (func (export "init") (param $seed i32)
    (local $x i32) (local $i i32) (local $n i32) (local $a i32)
    (local.set $x (i32.or (i32.mul (local.get $seed) (i32.const 2654435)) (i32.const 1)))
    (local.set $n (i32.add (i32.rem_u (i32.mul (local.get $seed) (i32.const 53)) (i32.const 1500)) (i32.const 1)))
    (local.set $a (i32.mul (i32.rem_u (local.get $seed) (i32.const 7)) (i32.const 4)))
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (local.get $n)))
      (local.set $x (call $xs (local.get $x)))
      (i32.store (i32.add (local.get $a) (i32.mul (local.get $i) (i32.const 4))) (local.get $x))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (if (i32.eqz (i32.rem_u (local.get $seed) (i32.const 5)))
      (then (drop (memory.grow (i32.const 1)))
            (i32.store (i32.add (i32.const 65536) (i32.mul (i32.rem_u (local.get $seed) (i32.const 100)) (i32.const 4)))
                       (local.get $x))))
    (global.set $g (local.get $x))
    (global.set $h (i64.add (i64.mul (i64.extend_i32_u (local.get $x)) (i64.const 3))
                            (i64.extend_i32_u (local.get $seed))))
    (memory.init $d (i32.const 8000) (i32.const 0) (i32.const 16))
    (data.drop $d)
    (table.set $t (i32.rem_u (local.get $seed) (i32.const 4)) (ref.func $f1))
    (if (i32.eqz (i32.rem_u (local.get $seed) (i32.const 3)))
      (then (drop (table.grow $t (ref.func $f2) (i32.rem_u (local.get $seed) (i32.const 6)))))))
  (func (export "step") (param $x i32) (result i32)
    (local $s i32)
    (local.set $s (i32.add (i32.load (i32.mul (i32.rem_u (local.get $x) (i32.const 7)) (i32.const 4)))
                           (i32.load (i32.mul (i32.rem_u (i32.mul (local.get $x) (i32.const 13)) (i32.const 1500)) (i32.const 4)))))
    (local.set $s (i32.add (local.get $s) (i32.add (global.get $g) (i32.wrap_i64 (global.get $h)))))
    (local.set $s (i32.add (local.get $s) (i32.mul (table.size $t) (i32.const 1000003))))
    (local.set $s (i32.add (local.get $s) (i32.load8_u (i32.add (i32.const 8000) (i32.rem_u (local.get $x) (i32.const 16))))))
    (i32.store (i32.mul (i32.rem_u (i32.mul (local.get $x) (i32.const 7)) (i32.const 2000)) (i32.const 4)) (local.get $s))
    (global.set $g (i32.add (global.get $g) (local.get $s)))
    (global.set $h (i64.add (i64.mul (global.get $h) (i64.const 3)) (i64.extend_i32_u (local.get $x))))
    (table.set $t (i32.rem_u (i32.add (local.get $x) (i32.const 1)) (i32.const 4)) (ref.func $f2))
    (i32.add (local.get $s) (call_indirect $t (type $v) (i32.rem_u (local.get $x) (i32.const 4)))))
  (func (export "scribble")
    (drop (memory.grow (i32.sub (i32.const 8) (memory.size))))
    (i32.store (i32.const 524284) (i32.const 0x5C81BB1E))
    (i32.store (i32.const 16) (i32.const 0x5C81BB1E))
    (global.set $g (i32.const 77))
    (drop (table.grow $t (ref.func $f0) (i32.const 5000)))
    (table.set $t (i32.const 0) (ref.null func)))
  (func (export "sum") (result i32)
    (local $s i32) (local $i i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (i32.const 2048)))
      (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (i32.load (i32.mul (local.get $i) (i32.const 4)))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31))
                           (i32.load (i32.sub (i32.mul (memory.size) (i32.const 65536)) (i32.const 4)))))
    (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (memory.size)))
    (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (global.get $g)))
    (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (i32.wrap_i64 (i64.rotl (global.get $h) (i64.const 17)))))
    (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (table.size $t)))
    (local.set $i (i32.const 0))
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (table.size $t)))
      (local.set $s (i32.mul (local.get $s) (i32.const 31)))
      (if (i32.eqz (ref.is_null (table.get $t (local.get $i))))
        (then (local.set $s (i32.add (local.get $s) (call_indirect $t (type $v) (local.get $i))))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (local.get $s))
  (func (export "growsum") (result i32)
    (local $p i32) (local $i i32) (local $s i32)
    (local.set $p (memory.grow (i32.const 1)))
    (if (i32.eq (local.get $p) (i32.const -1)) (then (return (i32.const -1))))
    (local.set $i (i32.mul (local.get $p) (i32.const 65536)))
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (i32.mul (memory.size) (i32.const 65536))))
      (local.set $s (i32.or (local.get $s) (i32.load (local.get $i))))
      (local.set $i (i32.add (local.get $i) (i32.const 4)))
      (br $l)))
    (i32.add (local.get $s) (local.get $p))))
"""

SEEDS = [[(i * 37 + 5) % 1000] for i in range(N)]
XS = [[(i * 11 + 3) % 257] for i in range(N)]
XS2 = [[(i * 29 + 1) % 263] for i in range(N)]
NONE = [[] for _ in range(N)]


def src_vectors():
    rng = np.random.RandomState(5)
    rot = [(i & ~63) + ((i & 63) + 1) % min(64, N - (i & ~63)) for i in range(N)]
    return {"all0": [0] * N, "all65": [65] * N, "all129": [129] * N, "reverse": [N - 1 - i for i in range(N)],
            "rotate": rot, "random": [int(v) for v in rng.randint(0, N // 2, N)]}


_wasm = None


def wasm():
    global _wasm
    if _wasm is None:
        _wasm = assemble(WAT)
    return _wasm


class Twins:
    """The oracle's instances, one per batch instance, driven in the same order."""

    def __init__(self, seeds=None, **kw):
        self.mod = O.Module(wasm())
        self.kw = kw
        self.inst = [O.Instance(self.mod, **kw) for _ in range(N)]
        if seeds is not None:
            self.call("init", seeds)

    def call(self, func, rows):
        return [t.invoke(func, row) for t, row in zip(self.inst, rows)]

    def fork(self, src, seeds=SEEDS):
        """twins of a batch restored through src from the state after init(seeds)"""
        return Twins([seeds[s] for s in src], **self.kw)


def pages(inst):
    return O.lib().om_mem_pages(inst._h)


def gpu_call(ctx, func, rows, nret):
    from wasmedge_amd import batch
    rets, st, cnt = ctx.execute(func, batch.make_values(rows, [I32] * len(rows[0])), nret)
    ints = batch.ret_ints(rets)
    return [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(ctx.n)], st, cnt


def check(ctx, twins, func, rows, nret, what):
    """run func on both sides; every instance equal in status, returns, counts, memory hash,
    pages and globals"""
    exp = twins.call(func, rows)
    rets, st, cnt = gpu_call(ctx, func, rows, nret)
    bad = compare(exp, rets, st, cnt, ctx.memory_hash(), [I32] * nret, exact=True)
    assert not bad, (what, func, bad[:5])
    for i, t in enumerate(twins.inst):
        assert ctx.memory_pages(i) == pages(t), (what, func, i, "pages")
        assert ctx.global_get("g", i)[0] == t.global_get(0), (what, func, i, "g")
        assert ctx.global_get("h", i)[0] == t.global_get(1), (what, func, i, "h")
    return st


def context(granule=4, **kw):
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, device=0, memory_granule=granule, **kw)
    assert ctx.memory_granule() == granule
    return ctx


# ---- CPU cases ----------------------------------------------------------------------------
def test_header_compiles_as_c(built, tmp_path):
    """the header beside the reference's wasmedge.h types, as a C translation unit"""
    src = tmp_path / "snap_abi.c"
    src.write_text('#include "wasmedge_batch.h"\n'
                   "WasmEdge_BatchSnapshot *take(WasmEdge_BatchContext *c, WasmEdge_Result *r) {\n"
                   "  return WasmEdge_BatchSnapshotCreate(c, r); }\n"
                   "WasmEdge_Result back(WasmEdge_BatchContext *c, const WasmEdge_BatchSnapshot *s, const uint32_t *m, double *t) {\n"
                   "  return WasmEdge_BatchSnapshotRestore(c, s, m, t); }\n"
                   "uint64_t size(const WasmEdge_BatchSnapshot *s) { return WasmEdge_BatchSnapshotGetBytes(s); }\n"
                   "void drop(WasmEdge_BatchSnapshot *s) { WasmEdge_BatchSnapshotDelete(s); }\n")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "snap_abi.o")])


def test_null_arguments(built):
    """through ctypes on the product library, no GPU touched"""
    from wasmedge_amd import batch
    L = batch.lib()
    res = batch._Result(0x55)
    assert L.WasmEdge_BatchSnapshotCreate(None, ctypes.byref(res)) is None
    assert res.Code == 0x04
    assert L.WasmEdge_BatchSnapshotRestore(None, None, None, None).Code == 0x04
    assert L.WasmEdge_BatchSnapshotGetBytes(None) == 0
    L.WasmEdge_BatchSnapshotDelete(None)


PLAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "snapshot_plan.h"
// stdin: n image_words mem_words same_granule has_src, then nwaves*64 marks, then n sources;
// stdout: rows, offsets, total, then per wave class and tiles, then the source of every lane
int main() {
  unsigned n, iw, mw, same, has;
  if (scanf("%u %u %u %u %u", &n, &iw, &mw, &same, &has) != 5) return 2;
  const unsigned nw = (n + 63) / 64;
  std::vector<uint32_t> marks(nw * 64), src(n), rows;
  std::vector<uint64_t> off;
  for (auto &m : marks) if (scanf("%u", &m) != 1) return 2;
  for (unsigned i = 0; i < n && has; i++) if (scanf("%u", &src[i]) != 1) return 2;
  const uint64_t total = wbs::pack_rows(marks.data(), nw, iw, mw, &rows, &off);
  for (unsigned w = 0; w < nw; w++) printf("%u %llu\n", rows[w], (unsigned long long)off[w]);
  printf("%llu\n", (unsigned long long)total);
  wbs::RestorePlan P;
  wbs::plan_restore(has ? src.data() : nullptr, n, nw, rows.data(), same != 0, &P);
  for (unsigned w = 0; w < nw; w++)
    printf("%u %u %u\n", P.wave[2 * w], P.wave[2 * w + 1], wbs::visit_tiles(P.wave[2 * w + 1], rows[nw - 1 - w]));
  for (unsigned i = 0; i < nw * 64; i++) printf("%u\n", P.src[i]);
  printf("%u %d\n", P.max_tiles, P.identity ? 1 : 0);
  return 0;
}
"""


def model_rows(mark, image_words, mem_words):
    """brute force: the smallest multiple of 64 rows that covers every byte below the mark and
    the image, within the layout"""
    need = max(-(-mark // 4), image_words if image_words <= mem_words else 0)
    r = 0
    while r < need and r < mem_words:
        r += 64
    return min(r, mem_words)


@pytest.fixture(scope="module")
def plan_prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "main.cpp").write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "wasmedge_amd", "csrc"), str(d / "main.cpp"), "-o", str(d / "plan")])
    return str(d / "plan")


@pytest.mark.parametrize("name", ["identity"] + sorted(src_vectors()))
@pytest.mark.parametrize("same", [1, 0])
def test_plan_against_model(plan_prog, name, same):
    mem_words, image_words = 2 * 16384, 70
    special = [0, 1, 255, 256, 257, mem_words * 4, mem_words * 4 - 1, 0xFFFFFFFF]
    rng = np.random.RandomState(11)
    nw = (N + 63) // 64
    # wave 0: random marks; wave 1: every special mark, the layout's end among them; wave 2:
    # the small ones (257 bytes: 65 words, the image's 70: two tiles)
    marks = [int(rng.randint(0, 9000)) if i >> 6 == 0 else special[i % 8] if i >> 6 == 1 else special[i % 5]
             for i in range(nw * 64)]
    src = None if name == "identity" else src_vectors()[name]
    text = "%d %d %d %d %d\n" % (N, image_words, mem_words, same, 0 if src is None else 1)
    text += " ".join(map(str, marks)) + "\n" + (" ".join(map(str, src)) if src else "") + "\n"
    out = subprocess.run([plan_prog], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [model_rows(max(marks[w * 64:(w + 1) * 64]), image_words, mem_words) for w in range(nw)]
    assert rows[0] % 64 == 0 and 0 < rows[0] < mem_words and rows[1] == mem_words and rows[2] == 128
    off = 0
    for w in range(nw):
        assert out[w].split() == [str(rows[w]), str(off)], (w, out[w])
        off += rows[w] * 64
    assert int(out[nw]) == off
    lanes = []
    for i in range(nw * 64):   # a lane past n follows lane 0 of its wave, keeping its lane
        s = i if src is None else src[i] if i < N else (src[i & ~63] & ~63) | (i & 63)
        lanes.append(s)
    biggest, ident = 0, True
    for w in range(nw):
        mine = lanes[w * 64:(w + 1) * 64]
        waves = {s >> 6 for s in mine}
        cls = 0 if same and mine == list(range(w * 64, w * 64 + 64)) else 1 if len(waves) == 1 else 2
        tiles = max(rows[v] for v in waves) // 64
        cur = rows[nw - 1 - w]   # (any current bound: the other end's rows)
        assert out[nw + 1 + w].split() == [str(cls), str(tiles), str(max(tiles, cur // 64))], (w, out[nw + 1 + w])
        biggest, ident = max(biggest, tiles), ident and cls == 0
    assert [int(v) for v in out[2 * nw + 1:2 * nw + 1 + nw * 64]] == lanes
    assert out[2 * nw + 1 + nw * 64].split() == [str(biggest), "1" if ident else "0"]


@pytest.mark.parametrize("image_words", [0, 1, 64, 65])
def test_plan_rows_per_mark(plan_prog, image_words):
    """a wave per mark: 0, 1, 255, 256, 257 bytes, the layout's end and past it"""
    mem_words = 16384
    special = [0, 1, 255, 256, 257, mem_words * 4 - 4, mem_words * 4 - 3, mem_words * 4, mem_words * 4 + 1, 0xFFFFFFFF]
    nw = len(special)
    marks = []
    for w in range(nw):
        marks += [0] * 17 + [special[w]] + [min(special[w], 3)] * 46
    text = "%d %d %d 1 0\n%s\n\n" % (nw * 64 - 9, image_words, mem_words, " ".join(map(str, marks)))
    out = subprocess.run([plan_prog], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    off = 0
    for w in range(nw):
        rows = model_rows(special[w], image_words, mem_words)
        assert out[w].split() == [str(rows), str(off)], (special[w], out[w])
        off += rows * 64
    assert int(out[nw]) == off


# ---- GPU cases ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("granule", GRANULES)
def test_round_trip(built, granule):
    """init, snapshot, step, restore, sum: the state after init alone; a second step equals
    the first; the snapshot restored twice"""
    ctx = context(granule)
    tw = Twins()
    check(ctx, tw, "init", SEEDS, 0, "init")
    snap = ctx.snapshot()
    assert snap.nbytes > 0
    first = Twins(SEEDS)
    st1 = check(ctx, first, "step", XS, 1, "first step")
    assert st1.any() and not st1.all()   # trapped instances are part of every comparison
    for k in range(2):
        ctx.restore(snap)
        with pytest.raises(Exception):   # results are as after a Reset: none until a run
            ctx.results(1)
        check(ctx, tw, "sum", NONE, 1, "sum after restore %d" % k)
        again = Twins(SEEDS)
        check(ctx, again, "step", XS, 1, "step after restore %d" % k)
    snap.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [4, 128])
def test_tail_reinitialised(built, granule):
    """scribble after the snapshot: a restore clears what lies above the snapshot's bound and
    brings the page counts and the table back; pages grown afterwards read zero"""
    ctx = context(granule)
    tw = Twins(SEEDS)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    _, st, _ = gpu_call(ctx, "scribble", NONE, 0)
    assert not st.any() and ctx.memory_pages(3) == 8 and ctx.table_size("t", 3) > 5000
    ctx.restore(snap)
    for i in (0, 64, 129):
        assert ctx.table_size("t", i) == 4 + (SEEDS[i][0] % 6 if SEEDS[i][0] % 3 == 0 else 0)
    check(ctx, tw, "sum", NONE, 1, "sum after scribble + restore")
    for k in range(3):
        check(ctx, tw, "growsum", NONE, 1, "growsum %d" % k)
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_restore_onto_lower_state(built):
    """snapshot, reset(), restore: nothing may rely on the current marks covering the snapshot"""
    ctx = context(4)
    tw = Twins(SEEDS)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    ctx.reset()
    ctx.restore(snap)
    check(ctx, tw, "sum", NONE, 1, "sum")
    check(ctx, tw, "step", XS, 1, "step")
    ctx.close()
    snap.close()   # (after its context: stays safe)


# memory and a global only (no per-instance table, 4-byte granules): the module whose untimed
# Reset is left to the next launch
PLAIN_WAT = r"""
(module
  (memory 1 2)
  (global $g (mut i32) (i32.const 5))
  (data (i32.const 12) "image")
  (func (export "fill") (param $s i32)
    (local $i i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (i32.rem_u (i32.mul (local.get $s) (i32.const 7)) (i32.const 900))))
      (i32.store (i32.mul (local.get $i) (i32.const 4)) (i32.mul (local.get $s) (i32.add (local.get $i) (i32.const 3))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (global.set $g (i32.add (global.get $g) (local.get $s))))
  (func (export "sum") (result i32)
    (local $s i32) (local $i i32)
    (block $d (loop $l
      (br_if $d (i32.ge_u (local.get $i) (i32.const 1024)))
      (local.set $s (i32.add (i32.mul (local.get $s) (i32.const 31)) (i32.load (i32.mul (local.get $i) (i32.const 4)))))
      (local.set $i (i32.add (local.get $i) (i32.const 1)))
      (br $l)))
    (i32.add (local.get $s) (global.get $g))))
"""


@pytest.mark.gpu
def test_deferred_reset(built):
    """a restore straight after reset(timed=False), before any run: the next run sees the
    snapshot, not the image; a snapshot straight after an untimed Reset is a fresh instance"""
    from wasmedge_amd import batch
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
    # the rows written (under 900 words a lane), not the memories (a page a lane)
    assert 0 < snap.nbytes < N * 65536 // 4
    gpu_call(ctx, "fill", XS, 0)
    ctx.reset(timed=False)
    ctx.restore(snap, timed=False)
    both(tw, "sum", NONE, 1, "sum after untimed reset + restore")
    both(tw, "fill", XS2, 0, "fill after it")
    ctx.reset(timed=False)
    fresh = ctx.snapshot()
    gpu_call(ctx, "fill", SEEDS, 0)
    ctx.restore(fresh, timed=False)
    tw = [O.Instance(mod) for _ in range(N)]
    both(tw, "sum", NONE, 1, "the snapshot of a reset state")
    both(tw, "fill", XS, 0, "fill on it")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("granule", [4, 128])
def test_fork(built, granule):
    """instance i from the captured instance src[i]; a second restore with another src from
    the same snapshot, with no Reset between"""
    ctx = context(granule)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    base = Twins()
    for name, src in src_vectors().items():
        ctx.restore(snap, src_of=src)
        tw = base.fork(src)
        check(ctx, tw, "sum", NONE, 1, name)
        check(ctx, tw, "step", XS, 1, name)
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_marks_after_fork(built):
    """restore a fork, reset(): every lane a fresh instance -- the destination's write mark
    is its source's"""
    ctx = context(4)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    ctx.restore(snap, src_of=src_vectors()["reverse"])
    ctx.reset()
    check(ctx, Twins(), "sum", NONE, 1, "sum after fork + reset")
    ctx.restore(snap, src_of=[N - 1] * N)   # (the heaviest of the partial wave everywhere)
    ctx.reset()
    check(ctx, Twins(), "sum", NONE, 1, "sum after broadcast + reset")
    ctx.close()


@pytest.mark.gpu
def test_errors(built):
    from wasmedge_amd import batch
    ctx, other = context(4), context(4)
    gpu_call(ctx, "init", SEEDS, 0)
    gpu_call(other, "init", SEEDS, 0)
    snap, foreign = ctx.snapshot(), other.snapshot()
    before = ctx.memory_hash()
    with pytest.raises(batch.WasmEdgeError) as e:
        ctx.restore(foreign)
    assert e.value.code == 0x04
    with pytest.raises(batch.WasmEdgeError) as e:
        ctx.restore(snap, src_of=[0] * (N - 1) + [N])
    assert e.value.code == 0x04
    with pytest.raises(ValueError):
        ctx.restore(snap, src_of=[0] * (N - 1))
    assert (ctx.memory_hash() == before).all()
    check(ctx, Twins(SEEDS), "step", XS, 1, "state untouched by refused restores")
    snap.close()
    assert snap.nbytes == 0
    with pytest.raises(ValueError):
        ctx.restore(snap)
    other.close()
    with pytest.raises(batch.WasmEdgeError) as e:   # its context is gone: inert
        ctx.restore(foreign)
    assert e.value.code == 0x04
    foreign.close()
    ctx.close()


@pytest.mark.gpu
def test_granule_changed_between_capture_and_restore(built):
    """mt19937 through the layout trial (as tests/test_layout.py drives it): a snapshot taken
    under 128-byte granules restored under 4-byte words, identity and one fork; exact"""
    from conftest import golden
    from wasmedge_amd import batch
    I64 = 0x7E
    w = golden("mt19937.wasm")
    rows = [[0, 5489 + 17 * i, 300 + i % 9] for i in range(N)]
    rows2 = [[0, 77 + i, 250 + i % 5] for i in range(N)]
    mod = O.Module(w)
    ctx = batch.BatchContext(w, N, device=0)

    def both(twins, rws, what):
        exp = [t.invoke("mt19937", r) for t, r in zip(twins, rws)]
        rets, st, cnt = ctx.execute("mt19937", batch.make_values(rws, [I32, I64, I64]), 1)
        ints = batch.ret_ints(rets)
        got = [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(N)]
        bad = compare(exp, got, st, cnt, ctx.memory_hash(), [I64], exact=True)
        assert not bad, (what, bad[:5])

    def twins_after(src):
        tw = [O.Instance(mod) for _ in range(N)]
        for t, s in zip(tw, src):
            t.invoke("mt19937", rows[s])
        return tw

    both([O.Instance(mod) for _ in range(N)], rows, "warm-up run")
    taken_under = ctx.memory_granule()
    snap = ctx.snapshot()
    ctx.reset()
    ctx.execute("mt19937", batch.make_values(rows, [I32, I64, I64]), 1)   # (measured)
    ctx.reset()                                                          # (switches)
    assert {taken_under, ctx.memory_granule()} == {128, 4}
    ctx.restore(snap)
    both(twins_after(range(N)), rows2, "identity under the other granule")
    src = src_vectors()["random"]
    ctx.restore(snap, src_of=src)
    both(twins_after(src), rows2, "fork under whichever granule holds now")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_reserved_layout_grown_since(built):
    """snapshot under two reserved pages, a run that grows the layout, restore"""
    ctx = context(4, memory_reserve_pages=2)
    tw = Twins(SEEDS)
    gpu_call(ctx, "init", SEEDS, 0)
    assert ctx.reserved_pages() == 2
    snap = ctx.snapshot()
    gpu_call(ctx, "scribble", NONE, 0)
    assert ctx.reserved_pages() >= 8
    ctx.restore(snap)
    check(ctx, tw, "sum", NONE, 1, "sum")
    check(ctx, tw, "growsum", NONE, 1, "growsum")
    check(ctx, tw, "step", XS, 1, "step")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_pool_rows_at_capture(built, monkeypatch):
    """instances hold pool rows: with the layout pinned the capture fails with 0x02 and a
    message and the context still runs; unpinned it takes the rows into the layout"""
    from wasmedge_amd import batch
    monkeypatch.setenv("WB_RELAYOUT", "0")
    ctx = context(4, memory_reserve_pages=2)
    tw = Twins(SEEDS)
    gpu_call(ctx, "init", SEEDS, 0)
    check(ctx, tw, "scribble", NONE, 0, "scribble")
    assert ctx.reserved_pages() == 2
    with pytest.raises(batch.WasmEdgeError) as e:
        ctx.snapshot()
    assert e.value.code == 0x02 and "reserved layout" in str(e.value)
    check(ctx, tw, "sum", NONE, 1, "the context still runs")
    monkeypatch.delenv("WB_RELAYOUT")
    snap = ctx.snapshot()
    assert ctx.reserved_pages() >= 8
    check(ctx, tw, "sum", NONE, 1, "after the layout took the rows")
    gpu_call(ctx, "step", XS, 1)
    ctx.restore(snap)
    check(ctx, tw, "step", XS2, 1, "step after restore")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_multi_memories(built):
    """three memories: run, snapshot, mutate all three and grow memory 1, restore; every
    memory folds into the results (tests/test_multimem.py's module). Identity and broadcast."""
    from test_multimem import MM_WAT
    from wasmedge_amd import batch
    w = assemble(MM_WAT)
    mod = O.Module(w, multi_memory=True)
    rows = [[i * 3 + 1, 20 + i % 40] for i in range(N)]
    rows2 = [[i * 5 + 2, 10 + i % 30] for i in range(N)]
    ctx = batch.BatchContext(w, N, device=0, multi_memory=True)

    def both(twins, rws, what):
        exp = [t.invoke("run", r) for t, r in zip(twins, rws)]
        rets, st, cnt = gpu_call(ctx, "run", rws, 1)
        bad = compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True)
        assert not bad, (what, bad[:5])

    def twins_after(src):
        tw = [O.Instance(mod) for _ in range(N)]
        for t, s in zip(tw, src):
            t.invoke("run", rows[s])
        return tw

    both([O.Instance(mod) for _ in range(N)], rows, "first run")
    snap = ctx.snapshot()
    gpu_call(ctx, "run", rows2, 1)
    ctx.restore(snap)
    both(twins_after(range(N)), rows2, "identity")
    ctx.restore(snap, src_of=[5] * N)
    both(twins_after([5] * N), rows2, "broadcast")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_metered(built):
    """the gas total is part of the state: equal to the capture's per instance, per source
    for a fork; a step that exceeds the limit does so at the oracle's instruction"""
    limit = 60000
    ctx = context(4, cost_limit=limit)
    tw = Twins(cost_limit=limit)
    check(ctx, tw, "init", SEEDS, 0, "init")
    at_capture = [t.cost_sum() for t in tw.inst]
    assert [int(c) for c in ctx.total_costs()] == at_capture
    snap = ctx.snapshot()
    gpu_call(ctx, "sum", NONE, 1)
    ctx.restore(snap)
    assert [int(c) for c in ctx.total_costs()] == at_capture
    st = check(ctx, tw, "sum", NONE, 1, "sum: some instances run out of gas")
    assert (st == 0x03).any() and (st == 0).any()
    assert [int(c) for c in ctx.total_costs()] == [t.cost_sum() for t in tw.inst]
    src = src_vectors()["reverse"]
    ctx.restore(snap, src_of=src)
    assert [int(c) for c in ctx.total_costs()] == [at_capture[s] for s in src]
    fk = Twins([SEEDS[s] for s in src], cost_limit=limit)
    check(ctx, fk, "sum", NONE, 1, "sum after a fork")
    snap.close()
    ctx.close()


@pytest.mark.gpu
def test_wasi_lane_state(built):
    """captured output and exit codes are the snapshot's; a broadcast of instance 3 gives
    every instance its output while an instance's own argv stays its own"""
    from test_wasi import ARGS, ENVS, WASI
    from wasmedge_amd import batch
    n = 96
    r1 = [[x] for x in range(n)]
    r2 = [[(x * 5 + 8) % 96] for x in range(n)]
    r3 = [[(x * 7) % 96] for x in range(n)]
    own = {7: ["seven", "x"], 40: ["forty"]}
    ctx = batch.BatchContext(WASI, n, device=0)
    ctx.init_wasi(ARGS, ENVS)
    for i, a in own.items():
        ctx.set_instance_args(i, a)
    O.set_wasi(True, ARGS, ENVS)
    try:
        mod = O.Module(WASI)

        def twins(first):
            """forked twins: the first run is the source's (the shared argv went into its
            memory), an instance's own argv counts from then on"""
            tw = [O.Instance(mod) for _ in range(n)]
            for i, t in enumerate(tw):
                t.invoke("run", first[i])
                if i in own:
                    t.set_args(own[i])
            return tw

        def side(tw):
            return [(t.wasi_output(1), t.wasi_output(2), t.wasi_exit_code()) for t in tw]

        def gpu_side():
            return [(ctx.wasi_output(i, 1), ctx.wasi_output(i, 2), ctx.wasi_exit_code(i)) for i in range(n)]

        def both(tw, rws, what):
            exp = [t.invoke("run", r) for t, r in zip(tw, rws)]
            rets, st, cnt = gpu_call(ctx, "run", rws, 1)
            bad = compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True)
            assert not bad, (what, bad[:5])
            assert gpu_side() == side(tw), what

        fresh = [O.Instance(mod) for _ in range(n)]
        for i, t in enumerate(fresh):
            if i in own:
                t.set_args(own[i])
        both(fresh, r1, "first run")
        snap = ctx.snapshot()
        gpu_call(ctx, "run", r2, 1)   # (more output, proc_exit on some)
        ctx.restore(snap)
        assert gpu_side() == side(fresh), "the snapshot's output and exit codes"
        both(fresh, r3, "run after restore")
        ctx.restore(snap, src_of=[3] * n)
        bc = twins([r1[3]] * n)
        assert gpu_side() == side(bc), "instance 3's output everywhere"
        both(bc, r3, "run after the broadcast (own argv stays)")
    finally:
        O.set_wasi(False)
    snap.close()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("part", [0, 1])
def test_two_shards(built, part):
    """two shards on one device: identity restore exact; a non-NULL SrcOf is refused with
    0x02 and a message, state untouched"""
    from wasmedge_amd import batch
    ctx = batch.BatchContext(wasm(), N, devices=[0, 0], partition=part)
    tw = Twins(SEEDS)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    assert snap.nbytes > 0
    gpu_call(ctx, "step", XS, 1)
    ctx.restore(snap)
    exp = tw.call("sum", NONE)
    rets, st, cnt = gpu_call(ctx, "sum", NONE, 1)
    assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True) == []
    before = ctx.memory_hash()
    with pytest.raises(batch.WasmEdgeError) as e:
        ctx.restore(snap, src_of=[0] * N)
    assert e.value.code == 0x02 and "multi-device" in str(e.value)
    assert (ctx.memory_hash() == before).all()
    exp = tw.call("step", XS)
    rets, st, cnt = gpu_call(ctx, "step", XS, 1)
    assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True) == []
    ctx.close()
    snap.close()   # (after its context and the shards: stays safe)


ENGINES = {   # tests/test_workloads.py's matrix for partial waves
    "simt": {}, "trip": {"WB_TRIP": "1"}, "nosimt": {"WB_SIMT": "0"}, "nojit": {"WB_JIT": "0"},
    "lds": {"WB_VFRAME": "0"}, "step": {"WB_THREADED": "0"}, "hbm": {"WB_HBMFRAME": "1"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_engines_after_restore(built, monkeypatch, engine):
    """every engine continues from a restored state: step above, and a small C2 (BLAKE3, few
    trips) whose chain runs from the restored memory"""
    from wasmedge_amd import batch, workloads as W
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)
    ctx = context(4)
    gpu_call(ctx, "init", SEEDS, 0)
    snap = ctx.snapshot()
    gpu_call(ctx, "step", XS2, 1)
    src = src_vectors()["rotate"]
    ctx.restore(snap, src_of=src)
    check(ctx, Twins().fork(src), "step", XS, 1, engine)
    snap.close()
    ctx.close()
    w = W.blake3_wasm()
    mod = O.Module(w)
    rows = [[i, 1 + i % 3] for i in range(N)]
    rows2 = [[i * 7 + 1, 2 + i % 2] for i in range(N)]
    ctx = batch.BatchContext(w, N, device=0)
    tw = [O.Instance(mod) for _ in range(N)]
    for t, r in zip(tw, rows):
        t.invoke("run", r)
    ctx.execute("run", batch.make_values(rows, [I32, I32]), 1)
    snap = ctx.snapshot()
    ctx.execute("run", batch.make_values(rows2, [I32, I32]), 1)
    ctx.restore(snap)
    exp = [t.invoke("run", r) for t, r in zip(tw, rows2)]
    rets, st, cnt = gpu_call(ctx, "run", rows2, 1)
    assert compare(exp, rets, st, cnt, ctx.memory_hash(), [I32], exact=True) == [], engine
    snap.close()
    ctx.close()
