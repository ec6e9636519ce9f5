"""Counted trips of a tight forwarding loop (jit.cpp RunCompile::counted_edge; DESIGN.md
"Compiled runs").

Where the back edge of a hoisted loop compares an i32 counter (written once per trip, as
i + constant) with a limit the loop never writes, and every lane of the group holds the
same counter and the same limit, the loop's head (Lhd) knows how many further trips
surely take the back edge. It clamps the count-down to that number and runs them in a
counted copy of the block (Lfc<p>): U trips of vector code back to back, one count-down
and one backward branch per pass, no compare. The tested loop keeps its text and runs
what is left. The static tests read the generated code; the GPU tests run uniform and
non-uniform groups, every compare kind, wrap-around, limits and the budget falling
inside a counted pass, against the oracle and bit for bit against WB_FWD_COUNT=0.

The oracle has no step limit, so it gives no count for a run that MaxSteps interrupts:
those runs are checked for status Interrupted, a count at or past the limit, and bit for
bit (counts included) against WB_FWD_COUNT=0; resumed to their end they are compared with
the oracle's uninterrupted run."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import oracle_py as O
from helpers import compare, gpu_run, jit_check
from test_chainloop import _asm_lines, _backward_branches, _counts, _modules, _steady_loop, chain_module
from wasmedge_amd import workloads as W
from wasmedge_amd.wat import assemble

I32 = 0x7F
INTERRUPTED = 0x07
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwdcount_off_sha256.json")

LEAF = r"""
  (memory 1)
  (func $leaf (param $out i32) (param $in i32) (param $a i32) (param $b i32) (param $c i32)
    (local $t i32) (local $u i32)
    (local.set $t (i32.load offset=0 (local.get $in)))
    (local.set $u (i32.load offset=4 (local.get $out)))
    (local.set $t (i32.xor (i32.rotl (i32.add (local.get $t) (local.get $a)) (i32.const 7)) (local.get $b)))
    (local.set $u (i32.add (i32.xor (local.get $u) (local.get $c)) (local.get $in)))
    (local.set $t (i32.add (i32.add (local.get $t) (local.get $out)) (local.get $u)))
    (local.set $u (i32.rotl (i32.xor (i32.or (local.get $u) (local.get $out)) (local.get $b)) (i32.const 13)))
    (i32.store offset=0 (local.get $out) (i32.add (local.get $t) (local.get $c)))
    (i32.store offset=4 (local.get $out) (i32.xor (local.get $u) (local.get $t))))
  (func $sum (result i32)
    (i32.add (i32.load (i32.const 0)) (i32.load (i32.const 4))))
  (func (export "nop"))
"""


def loop_module(cond="(i32.lt_u (local.get $i) (local.get $n))", step="(i32.const 1)", extra="",
                leaf=LEAF, arg="(local.get $i)"):
    """run(s, n, i): test_chainloop.chain_module's loop as a do-while from a given start:
    leaf(0, 64, -1, 0xdeadbeef, i); i += step; back while `cond`. `extra` goes before the
    counter's update. ($pad: the callee's cells start an even number of cells above the
    frame base.)"""
    return assemble(r"""
(module %s
  (func (export "run") (param $s i32) (param $n i32) (param $i i32) (result i32)
    (local $pad i32)
    (i32.store (i32.const 64) (local.get $s))
    (i32.store (i32.const 4) (i32.mul (local.get $s) (i32.const 40503)))
    (loop $chain
      (call $leaf (i32.const 0) (i32.const 64) (i32.const -1) (i32.const 0xdeadbeef) %s)
      %s
      (local.set $i (i32.add (local.get $i) %s))
      (br_if $chain %s))
    (i32.add (call $sum) (local.get $i))))
""" % (leaf, arg, extra, step, cond))


LT_U = loop_module()
LT_S = loop_module("(i32.lt_s (local.get $i) (local.get $n))")
GT_U = loop_module("(i32.gt_u (local.get $n) (local.get $i))", "(i32.const 2)")
NE3 = loop_module("(i32.ne (local.get $i) (local.get $n))", "(i32.const 3)")
NE_DOWN = loop_module("(i32.ne (local.get $i) (local.get $n))", "(i32.const -1)")
UNLESS = loop_module("(i32.eqz (i32.ge_u (local.get $i) (local.get $n)))")   # eqz + br_if: BR_UNLESS
LT_IMM = loop_module("(i32.lt_u (local.get $i) (i32.const 11))")
COUNTED = {"lt_u": LT_U, "lt_s": LT_S, "gt_u": GT_U, "ne3": NE3, "ne_down": NE_DOWN, "unless": UNLESS,
           "lt_imm": LT_IMM}


def _dump(wasm, flavour="simt"):
    return _asm_lines(jit_check(wasm, 0, dump=flavour)[2])


def _counted(lines):
    """the counted copy: from its label to the branch back to it (None without one)"""
    heads = [i for i, ln in enumerate(lines) if re.fullmatch(r"Lfc\d+p:", ln)]
    if not heads:
        return None
    assert len(heads) == 1, heads
    lab = lines[heads[0]][:-1]
    back = [i for i, ln in enumerate(lines)
            if i > heads[0] and ln.startswith("s_cbranch") and ln.split()[-1] == lab]
    assert len(back) == 1, back
    return lines[heads[0]:back[0] + 1]


def _unroll():
    """U of the default build, read from the counted copy's count-down"""
    cut = _counted(_dump(chain_module()))
    m = re.fullmatch(r"s_sub_u32 s100, s100, (\d+)", cut[-2])
    assert m, cut[-2:]
    return int(m.group(1))


def _valu(cut):
    return [ln for ln in cut if ln.startswith("v_")]


# ---------------------------------------------------------------- static
@pytest.mark.parametrize("unroll", [None, 1, 2, 4])
def test_counted_copy_of_blake3(built, monkeypatch, unroll):
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    monkeypatch.delenv("WB_FWD_UNROLL", raising=False)
    if unroll:
        monkeypatch.setenv("WB_FWD_UNROLL", str(unroll))
    U = unroll or _unroll()
    assert U in (1, 2, 4)
    lines = _dump(W.blake3_wasm())
    cut = _counted(lines)
    assert cut is not None
    tested = _steady_loop(W.blake3_wasm())
    assert len(_valu(cut)) == U * (len(_valu(tested)) - 1)
    assert not [ln for ln in cut if ln.startswith("v_cmp") or "vcc" in ln], cut
    assert not [ln for ln in cut if ln.startswith(("global_", "ds_", "buffer_", "scratch_", "flat_", "s_load"))]
    assert len(_backward_branches(cut)) == 1
    # a pass: the trips' vector code, then the count-down and the branch alone
    other = [ln for ln in cut if not ln.startswith("v_") and not ln.endswith(":") and not ln.startswith(".")]
    assert other == ["s_sub_u32 s100, s100, %d" % U, "s_cbranch_scc0 " + cut[0][:-1]], other
    assert not re.fullmatch(r"Lb\d+c:", cut[0])
    # the trip's code is the tested block's but for its compare
    body = [ln for ln in _valu(tested) if not ln.startswith("v_cmp")]
    assert _valu(cut) == body * U


def test_tested_loop_is_unchanged(built, monkeypatch):
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    on = _steady_loop(W.blake3_wasm())
    assert sum(c for k, c in _counts(on).items() if k.startswith("v_")) <= 682
    monkeypatch.setenv("WB_FWD_COUNT", "0")
    assert on == _steady_loop(W.blake3_wasm())


@pytest.mark.parametrize("name", sorted(COUNTED))
def test_every_supported_edge_is_counted(built, monkeypatch, name):
    """lt_u, lt_s and ne with a constant step, either operand order, the br_unless lowering
    and a constant limit; plain and SIMT code alike"""
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    for flavour in ("plain", "simt"):
        assert _counted(_dump(COUNTED[name], flavour)) is not None, (name, flavour)
    assert _counted(_dump(chain_module())) is not None


def test_switched_off_every_module_is_as_before(built, monkeypatch):
    """WB_FWD_COUNT=0: the generated text of every flavour of every workload module, at
    granule logs 0, 2 and 5, is the one recorded (tests/golden) from the code generator
    before counted trips"""
    monkeypatch.setenv("WB_FWD_COUNT", "0")
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {}
    for name, wasm in _modules().items():
        for glog in (0, 2, 5):
            text = jit_check(wasm, glog, dump=("plain", "simt", "trip"))[2]
            for k in sorted(text):
                got["%s/%s/g%d" % (name, k, glog)] = hashlib.sha256(text[k].encode()).hexdigest()
    assert got == want


def test_off_with_the_hoisted_tail(built, monkeypatch):
    monkeypatch.setenv("WB_FWD_TAIL", "0")
    assert _counted(_dump(W.blake3_wasm())) is None


I64_COUNTER = assemble(r"""
(module %s
  (func (export "run") (param $s i32) (param $n i64) (result i32)
    (local $i i64)
    (loop $chain
      (call $leaf (i32.const 0) (i32.const 64) (i32.const -1) (i32.const 0xdeadbeef) (i32.wrap_i64 (local.get $i)))
      (local.set $i (i64.add (local.get $i) (i64.const 1)))
      (br_if $chain (i64.lt_u (local.get $i) (local.get $n))))
    (call $sum)))
""" % LEAF)

TRAPPING_LEAF = LEAF.replace("(i32.load offset=0 (local.get $in))", "(i32.load offset=0 (local.get $c))")

INELIGIBLE = {
    "limit written": loop_module(extra="(local.set $n (i32.xor (local.get $n) (local.get $s)))"),
    "i64 counter": I64_COUNTER,
    "step from memory": loop_module(step="(i32.load (i32.const 128))"),
    "step from a local": loop_module(step="(local.get $s)"),
    "counter written twice": loop_module(extra="(local.set $i (i32.add (local.get $i) (i32.const 1)))"),
    "le_u": loop_module("(i32.le_u (local.get $i) (local.get $n))"),
    "lt_u, stepping down": loop_module(step="(i32.const -1)"),
    "trapping load": loop_module(leaf=TRAPPING_LEAF),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_ineligible_loops_have_no_counted_copy(built, monkeypatch, name):
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    assert TRAPPING_LEAF != LEAF
    for flavour in ("plain", "simt"):
        lines = _dump(INELIGIBLE[name], flavour)
        assert _counted(lines) is None, (name, flavour)
        assert not [ln for ln in lines if ln.startswith(("Lfc", "Lhn"))]


def test_metered_context_has_no_counted_copy(built, monkeypatch):
    """(WB_JIT_CHECK_COST: the hook compiles the runs as a metered context does)"""
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    assert _counted(_dump(LT_U, "plain")) is not None
    monkeypatch.setenv("WB_JIT_CHECK_COST", "1")
    for wasm in (LT_U, chain_module(), W.blake3_wasm()):
        lines = _dump(wasm, "plain")
        assert lines and _counted(lines) is None


# ---------------------------------------------------------------- GPU parity
_REF = {}
SIZES = [64, 65, 130]   # one wave, a one-lane second wave, a partial third


def _oracle(wasm, func, rows):
    """one oracle pass per distinct call, shared by every test"""
    m = None
    out = []
    for r in rows:
        key = (wasm, func, tuple(r))
        if key not in _REF:
            m = m or O.Module(wasm)
            _REF[key] = m.run(func, list(r))
        out.append(_REF[key])
    return out


def _on_off(monkeypatch, run):
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    on = run()
    monkeypatch.setenv("WB_FWD_COUNT", "0")
    off = run()
    monkeypatch.delenv("WB_FWD_COUNT", raising=False)
    assert on[0] == off[0]
    for x, y in zip(on[1:], off[1:]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    return on


def _parity(monkeypatch, wasm, rows, **kw):
    ptypes = [I32] * len(rows[0])
    ref = _oracle(wasm, "run", rows)
    on = _on_off(monkeypatch, lambda: gpu_run(wasm, "run", rows, ptypes, [I32], **kw))
    assert compare(ref, *on, [I32], exact=True) == []
    return on


def _seed(i):
    return (i * 2654435761 + 7) & 0xFFFFFFFF


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_uniform_trip_counts(built, monkeypatch, n):
    U = _unroll()
    for trips in sorted({0, 1, 2, U - 1, U, U + 1, 2 * U, 2 * U + 1, 13}):
        _parity(monkeypatch, chain_module(), [[_seed(i), trips] for i in range(n)])
        _parity(monkeypatch, W.blake3_wasm(), [[i, trips] for i in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_limits_differ_by_lane(built, monkeypatch, n):
    """id mod 7: no lane group is uniform until lanes have left; 9 and 5 by halves: the
    lanes at 5 leave and the rest go on as a uniform group"""
    for wasm, arg in ((chain_module(), _seed), (W.blake3_wasm(), lambda i: i)):
        _parity(monkeypatch, wasm, [[arg(i), i % 7] for i in range(n)])
        _parity(monkeypatch, wasm, [[arg(i), 9 if i % 64 < 32 else 5] for i in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_uniform_limit_starts_differ_by_lane(built, monkeypatch, n):
    _parity(monkeypatch, LT_U, [[_seed(i), 20, i % 5] for i in range(n)])
    _parity(monkeypatch, NE_DOWN, [[_seed(i), 3, 10 + i % 3] for i in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_signedness_and_wrap(built, monkeypatch, n):
    M = 0xFFFFFFFF
    cases = [
        (LT_U, M, M - 15),         # n = 0xFFFFFFFF: the counter stops one short of wrapping
        (LT_U, 0, 0),              # n = 0: one trip
        (LT_U, 0, M - 3),          # ... from a start above it
        (LT_U, 5, M),              # the counter wraps to 0 and goes on to 5
        (LT_S, -5 & M, -20 & M),   # negative limit
        (LT_S, 6, -7 & M),         # negative start
        (LT_S, 0x80000000, 3),     # the lowest limit: one trip
        (LT_S, 0x7FFFFFFF, 0x7FFFFFF0),
        (GT_U, 21, 0),             # step 2, operands the other way round
        (GT_U, M, M - 8),          # step 2 up to n = 0xFFFFFFFF itself
        (NE3, 30, 0),              # step 3 onto the limit
        (NE3, 2, -10 & M),         # ... across zero
        (NE_DOWN, 0, 17),          # a count-down to zero
        (UNLESS, 14, 1),
        (LT_IMM, 0, 0),
        (LT_IMM, 0, 30),
    ]
    for wasm, lim, start in cases:
        _parity(monkeypatch, wasm, [[_seed(i), lim, start] for i in range(n)])


def _interrupted(on, limit):
    rets, st, cnt, h = on
    assert all(int(s) == INTERRUPTED for s in st), sorted(set(int(s) for s in st))
    assert int(min(cnt)) >= limit


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_ne_steps_over_its_limit(built, monkeypatch, n):
    """i = 0, 3, 6, ... never equals 4: the loop only ends at MaxSteps"""
    limit = 5000
    rows = [[_seed(i), 4, 0] for i in range(n)]
    on = _on_off(monkeypatch, lambda: gpu_run(NE3, "run", rows, [I32] * 3, [I32], max_steps=limit))
    _interrupted(on, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_max_steps_inside_a_counted_pass(built, monkeypatch, n):
    from wasmedge_amd import batch
    for wasm, rows, limit in ((chain_module(), [[_seed(i), 200] for i in range(n)], 3001),
                              (W.blake3_wasm(), [[i, 50] for i in range(n)], 50001)):
        ptypes = [I32] * 2
        ref = _oracle(wasm, "run", rows)
        assert min(r[2] for r in ref) > 2 * limit
        on = _on_off(monkeypatch, lambda: gpu_run(wasm, "run", rows, ptypes, [I32], max_steps=limit))
        _interrupted(on, limit)

        def resumed():
            ctx = batch.BatchContext(wasm, n, max_steps=limit, resumable=True)
            try:
                ctx.set_args("run", batch.make_values(rows, ptypes))
                ctx.run()
                mid = ctx.results(1)
                assert ctx.suspended() == n
                ctx.resume(0)
                assert ctx.suspended() == 0
                rets, st, cnt = ctx.results(1)
                ints = batch.ret_ints(rets)
                out = [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(n)]
                return out, st, cnt, ctx.memory_hash(), mid[1], mid[2]
            finally:
                ctx.close()

        got = _on_off(monkeypatch, resumed)
        assert all(int(x) == INTERRUPTED for x in got[4]) and int(min(got[5])) >= limit
        assert compare(ref, *got[:4], [I32], exact=True) == []


@pytest.mark.gpu
def test_gpu_outlasts_the_core_budget(built, monkeypatch):
    """64 x 450 compressions, about 1.2e6 instructions a lane: the budget (2^20) runs out
    inside the counted copy's share and the loop comes back through R and Lhd"""
    rets, st, cnt, h = _parity(monkeypatch, W.blake3_wasm(), [[i, 450] for i in range(64)])
    assert int(min(cnt)) > 1 << 20 and all(int(s) == 0 for s in st)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_half_the_lanes_sit_out(built, monkeypatch, n):
    """per-instance calls: odd lanes make no call"""
    from wasmedge_amd import batch
    func_of = [0 if i % 2 == 0 else None for i in range(n)]
    rows = [[(_seed(i), I32), (12, I32), (1, I32)] if i % 2 == 0 else [] for i in range(n)]
    fresh = _oracle(LT_U, "nop", [[]])[0][3]
    ref = [_oracle(LT_U, "run", [[v for v, _ in rows[i]]])[0] if i % 2 == 0 else (0, [], 0, fresh)
           for i in range(n)]

    def run():
        ctx = batch.BatchContext(LT_U, n, device=0)
        try:
            rets, st, cnt = ctx.execute_calls(["run"], func_of, rows)
            return rets, st, cnt, ctx.memory_hash()
        finally:
            ctx.close()

    on = _on_off(monkeypatch, run)
    assert compare(ref, *on, None, exact=True) == []
