"""The steady-state code of a forwarding loop (jit.cpp "Loop-carried memory forwarding",
"constant and copy propagation"; DESIGN.md "Compiled runs").

C2's chain loop runs in one compiled block: the forwarding copy Lb<R>c of the run that
calls the inlined compression and, right behind it, the post-call copy's code past its
POST_CALL, whose taken branch is the loop's one back edge. With the three switches on
(WB_KPROP: deferred constants and copies, WB_FWD_LAZY: the copy's stores stay in their
registers until the loop is left, WB_FWD_LOOP: no stack check, jump or second count per
trip) that block is BLAKE3's own 680 integer instructions plus the loop counter and its
compare. The static tests read the generated code; the GPU tests run loops whose lanes
leave at different trips, never enter the copy, or outlast the core's budget, against
the oracle and bit for bit against the switches off."""
import collections
import re

import numpy as np
import pytest

import oracle_py as O
from conftest import golden
from helpers import compare, gpu_run, jit_check
from wasmedge_amd import workloads as W
from wasmedge_amd.wat import assemble

I32 = 0x7F
SWITCHES = ("WB_KPROP", "WB_FWD_LAZY", "WB_FWD_LOOP")


def _asm_lines(src):
    return [m.group(1) for m in (re.match(r'\s*"(.*)\\n"\s*$', ln) for ln in src.splitlines()) if m]


def _steady_loop(wasm):
    """the lines from label Lb<R>c to the s_cbranch that returns to it"""
    lines = _asm_lines(jit_check(wasm, 0, dump="simt")[2])
    heads = [i for i, ln in enumerate(lines) if re.fullmatch(r"Lb\d+c:", ln)]
    assert len(heads) == 1, heads
    lab = lines[heads[0]][:-1]
    back = [i for i, ln in enumerate(lines)
            if i > heads[0] and ln.startswith("s_cbranch") and ln.split()[-1] == lab]
    assert back, "no branch back to " + lab
    return lines[heads[0]:back[0] + 1]


def _counts(cut):
    return collections.Counter(ln.split()[0] for ln in cut if not ln.endswith(":") and not ln.startswith("."))


def _backward_branches(cut):
    at = {ln[:-1]: i for i, ln in enumerate(cut) if ln.endswith(":")}
    return [ln for i, ln in enumerate(cut)
            if re.match(r"s_c?branch", ln) and at.get(ln.split()[-1], len(cut)) <= i]


def test_steady_state_loop_is_blake3_alone(built, monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    cut = _steady_loop(W.blake3_wasm())
    n = _counts(cut)
    assert n["v_mov_b32"] == 0, n
    assert not [k for k in n if k.startswith(("global_store", "global_load"))], n
    # (64-bit address arithmetic: shifts and adds on register pairs)
    assert not [ln for ln in cut if ln.startswith("v_") and ("_b64" in ln or "_u64" in ln)], n
    valu = sum(c for k, c in n.items() if k.startswith("v_"))
    assert valu <= 682, (valu, n)   # 7 rounds x 8 G x 12 + 8 output xors + counter + compare
    assert len(_backward_branches(cut)) == 1, _backward_branches(cut)


def test_loop_with_the_switches_off(built, monkeypatch):
    """the code before these switches, by instruction class (the cut then spans the p
    copy's head as well, which no trip runs: its v_subrev_u32 and v_lshl_add_u32 are the
    two VALU lines beyond the 703 below)"""
    for v in SWITCHES:
        monkeypatch.setenv(v, "0")
    n = _counts(_steady_loop(W.blake3_wasm()))
    cmp3 = sum(c for k, c in n.items() if k.startswith("v_cmp"))
    got = (n["v_xor_b32_e32"], n["v_alignbit_b32"], n["v_add_u32_e32"], n["v_add3_u32"],
           n["v_mov_b32"], n["v_lshlrev_b64"], n["v_lshl_add_u64"], cmp3)
    assert got == (232, 224, 114, 112, 16, 1, 1, 3), n
    assert sum(got) == 703
    assert n["global_store_dword"] == 8, n


def _modules():
    mods = {name: getattr(W, name)() for name in sorted(dir(W))
            if name.endswith("_wasm") and name != "blake3_kat_wasm"}
    mods["blake3_kat"] = W.blake3_kat_wasm(b"abc")
    mods["mt19937"] = golden("mt19937.wasm")
    mods["chain"] = chain_module()
    return mods


@pytest.mark.parametrize("glog", [0, 2, 5])
def test_every_flavour_assembles(built, monkeypatch, glog):
    """plain, SIMT and trip code of every workload module (jit_check fails with the
    assembler's message)"""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for name, wasm in _modules().items():
        runs, _, _ = jit_check(wasm, glog)
        assert runs >= 0, (name, glog)


def chain_module():
    """A chain loop round a leaf (out, in, a, b, c) called with the constants 0, 64, -1,
    0xdeadbeef and the loop counter: an address that is 0, an inline constant, a literal
    that is also the inline -1, a 32-bit literal, x + 0 / x ^ 0 / x | 0. The words the
    leaf stores are read by another function once the loop is left. ($pad: an inlined
    callee's cells start an even number of cells above the frame base.)"""
    return assemble(r"""
(module
  (memory 1)
  (func $leaf (param $out i32) (param $in i32) (param $a i32) (param $b i32) (param $c i32)
    (local $t i32) (local $u i32)
    (local.set $t (i32.load offset=0 (local.get $in)))
    (local.set $u (i32.load offset=4 (local.get $out)))
    (local.set $t (i32.xor (i32.rotl (i32.add (local.get $t) (local.get $a)) (i32.const 7)) (local.get $b)))
    (local.set $u (i32.add (i32.xor (local.get $u) (local.get $c)) (local.get $in)))
    (local.set $t (i32.add (i32.add (local.get $t) (local.get $out)) (local.get $u)))
    (local.set $u (i32.rotl (i32.xor (i32.or (local.get $u) (local.get $out)) (local.get $b)) (i32.const 13)))
    (local.set $u (i32.xor (local.get $u) (i32.xor (local.get $a) (local.get $out))))
    (i32.store offset=0 (local.get $out) (i32.add (local.get $t) (local.get $c)))
    (i32.store offset=4 (local.get $out) (i32.xor (local.get $u) (local.get $t))))
  (func $sum (result i32)
    (i32.add (i32.load (i32.const 0)) (i32.load (i32.const 4))))
  (func (export "run") (param $s i32) (param $n i32) (result i32)
    (local $i i32) (local $pad i32)
    (i32.store (i32.const 64) (local.get $s))
    (i32.store (i32.const 4) (i32.mul (local.get $s) (i32.const 40503)))
    (block $end
      (br_if $end (i32.eqz (local.get $n)))
      (loop $chain
        (call $leaf (i32.const 0) (i32.const 64) (i32.const -1) (i32.const 0xdeadbeef) (local.get $i))
        (local.set $i (i32.add (local.get $i) (i32.const 1)))
        (br_if $chain (i32.lt_u (local.get $i) (local.get $n)))))
    (call $sum)))
""")


def test_chain_module_forwards(built):
    cut = _steady_loop(chain_module())
    n = _counts(cut)
    assert not [k for k in n if k.startswith("global_")], n
    # the five arguments cost nothing: -1 and 0xdeadbeef are literals, 64 and 0 fold
    assert sum(1 for ln in cut if "0xdeadbeef" in ln) == 2 and n["v_mov_b32"] <= 1, cut
    assert len(_backward_branches(cut)) == 1


# ---------------------------------------------------------------- GPU parity
_REF = {}


def _oracle(key, wasm, rows):
    """one oracle pass per case, shared by the tests that need it"""
    if key not in _REF:
        m = O.Module(wasm)
        _REF[key] = [m.run("run", r) for r in rows]
    return _REF[key]


def _parity(monkeypatch, key, wasm, rows):
    """status, return value, instruction count and memory hash: against the oracle with the
    switches on, and the switches off bit for bit the same"""
    ref = _oracle(key, wasm, rows)
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    on = gpu_run(wasm, "run", rows, [I32, I32], [I32])
    assert compare(ref, *on, [I32], exact=True) == [], key
    for v in SWITCHES:
        monkeypatch.setenv(v, "0")
    off = gpu_run(wasm, "run", rows, [I32, I32], [I32])
    assert on[0] == off[0], key
    for x, y in zip(on[1:], off[1:]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), key
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 200])
def test_gpu_blake3_lanes_leave_at_different_trips(built, monkeypatch, n):
    rows = [[i, 1 + i % 7] for i in range(n)]
    _parity(monkeypatch, ("b3div", n), W.blake3_wasm(), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [0, 1])
def test_gpu_blake3_copy_not_entered_or_left_at_once(built, monkeypatch, iters):
    rows = [[i, iters] for i in range(65)]
    _parity(monkeypatch, ("b3", iters), W.blake3_wasm(), rows)


@pytest.mark.gpu
def test_gpu_blake3_outlasts_the_budget(built, monkeypatch):
    """64 x 300 compressions: about 7.8e5 instructions a lane, several budgets of the
    core -- the count-limit exit stores the dirty words and the loop resumes from memory"""
    rows = [[i, 300] for i in range(64)]
    rets, st, cnt, h = _parity(monkeypatch, "b3long", W.blake3_wasm(), rows)
    assert int(min(cnt)) > 700000


@pytest.mark.gpu
def test_gpu_blake3_long_run_completes(built, monkeypatch):
    """the same run with the interrupt left alone ends with every lane done"""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    rows = [[i, 300] for i in range(64)]
    ref = _oracle("b3long", W.blake3_wasm(), rows)
    rets, st, cnt, h = gpu_run(W.blake3_wasm(), "run", rows, [I32, I32], [I32])
    assert all(int(s) == 0 for s in st)
    assert compare(ref, rets, st, cnt, h, [I32], exact=True) == []


@pytest.mark.gpu
def test_gpu_chain_module_constants_and_exit_memory(built, monkeypatch):
    rows = [[(i * 2654435761 + 7) & 0xFFFFFFFF, i % 5] for i in range(65)]
    _parity(monkeypatch, "chain", chain_module(), rows)
