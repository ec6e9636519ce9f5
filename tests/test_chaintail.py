"""The tail of a tight forwarding loop (jit.cpp RunCompile::hoist; DESIGN.md "Compiled
runs").

LOW, OTHER and the count limit do not change while a group stays in the loop, so the
tests on them run once where the loop is entered (Lhd: it also turns the limit into a
trip count-down and adds those trips to CNT at once); a trip then ends in four scalar
instructions: VCC against EXEC, the branch to the full tail, the count-down and the back
edge. Every other way out takes the trips not run off CNT again. The static tests read
the generated code; the GPU tests leave the loop every way there is -- the budget, lanes
at different trips, a partial wave, lanes waiting at other pcs, MaxSteps, a gas limit --
against the oracle and bit for bit against WB_FWD_TAIL=0."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_py as O
from helpers import compare, gpu_run, jit_check
from test_chainloop import _backward_branches, _counts, _modules, _steady_loop, chain_module
from wasmedge_amd import workloads as W

I32 = 0x7F
KNOBS = ("WB_FWD_TAIL",)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chaintail_off_sha256.json")

# the steady block's scalar code with WB_FWD_TAIL=0 (C2)
OLD_TAIL = """s_mov_b32 s62, 0x2a60
s_and_b64 s[74:75], vcc, exec
s_cbranch_scc0 Lnt9p
s_cmp_eq_u64 s[74:75], exec
s_cbranch_scc0 Lbs9p
s_add_u32 s65, s65, 0xa32
s_cmp_ge_u32 s95, 0x2960
s_cselect_b32 s63, s95, s63
s_cmp_lt_u32 s65, s64
s_cselect_b32 s68, s63, 0
s_cmp_gt_u32 s68, 0x2a40
s_cbranch_scc1 Lb8c""".splitlines()


def _split(cut):
    code = [ln for ln in cut if not ln.endswith(":") and not ln.startswith(".")]
    return [ln for ln in code if ln.startswith("v_")], [ln for ln in code if not ln.startswith("v_")]


@pytest.mark.parametrize("name", ["blake3", "chain"])
def test_trip_ends_in_four_scalar_instructions(built, monkeypatch, name):
    monkeypatch.delenv("WB_FWD_TAIL", raising=False)
    monkeypatch.delenv("WB_FWD_LOOP", raising=False)
    cut = _steady_loop(W.blake3_wasm() if name == "blake3" else chain_module())
    valu, other = _split(cut)
    assert len(valu) <= 681, len(valu)
    assert len(other) <= 4, other
    assert len(_backward_branches(cut)) == 1, _backward_branches(cut)
    # the count-down is the only scalar register the block writes
    assert [ln.split()[0] for ln in other] == ["s_cmp_eq_u64", "s_cbranch_scc0", "s_add_u32", "s_cbranch_scc1"]
    assert other[2] == "s_add_u32 s100, s100, -1", other


def test_switched_off_the_tail_is_the_old_one(built, monkeypatch):
    monkeypatch.setenv("WB_FWD_TAIL", "0")
    valu, other = _split(_steady_loop(W.blake3_wasm()))
    assert other == OLD_TAIL
    assert len(valu) <= 681


def test_tail_needs_the_tight_loop(built, monkeypatch):
    """WB_FWD_LOOP=0 turns the hoisted tail off with it"""
    monkeypatch.setenv("WB_FWD_LOOP", "0")
    a = jit_check(W.blake3_wasm(), 0, dump="simt")[2]
    monkeypatch.setenv("WB_FWD_TAIL", "0")
    assert a == jit_check(W.blake3_wasm(), 0, dump="simt")[2]
    assert "s100" not in a


def test_switched_off_every_module_is_as_before(built, monkeypatch):
    """WB_FWD_TAIL=0: the generated text of every flavour of every workload module is the
    one recorded (tests/golden) from the code generator before the hoisted tail"""
    monkeypatch.setenv("WB_FWD_TAIL", "0")
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {}
    for name, wasm in _modules().items():
        text = jit_check(wasm, 0, dump=("plain", "simt", "trip"))[2]
        for k in sorted(text):
            got[name + "/" + k] = hashlib.sha256(text[k].encode()).hexdigest()
    assert got == want


def test_stall_model_with_the_measured_latencies(built, monkeypatch):
    """The static issue model (stall_model.py) on C2's steady block. With the measured
    table -- 4 cycles from any of the loop's instructions to any use, the issue interval --
    no instruction waits for a producer: fewer than 40 stall cycles per trip, the bound
    under which the list scheduler stays as it is. (At the 12 cycles the scheduler assumes
    the same order stalls little, at 16 it would stall every group: the order sits on 12.)"""
    import stall_model
    monkeypatch.delenv("WB_FWD_TAIL", raising=False)
    cut = _steady_loop(W.blake3_wasm())
    got = {L: stall_model.stall_cycles(cut, lambda p, c, L=L: L) for L in (12, 16)}
    measured = stall_model.stall_cycles(cut)
    print("stall cycles per trip: measured table %d, L=12 %d, L=16 %d" % (measured, got[12], got[16]))
    assert measured < 40
    assert got[12] < got[16]


# ---------------------------------------------------------------- GPU parity
_REF = {}


def _ref(key, make):
    """one oracle pass per case, shared by the tests that need it"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _on_off(monkeypatch, run):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    on = run()
    for v in KNOBS:
        monkeypatch.setenv(v, "0")
    off = run()
    assert on[0] == off[0]
    for x, y in zip(on[1:], off[1:]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    return on


def _parity(monkeypatch, key, wasm, rows, **kw):
    m = O.Module(wasm)
    ref = _ref(key, lambda: [m.run("run", r) for r in rows])
    on = _on_off(monkeypatch, lambda: gpu_run(wasm, "run", rows, [I32, I32], [I32], **kw))
    assert compare(ref, *on, [I32], exact=True) == [], key
    return on


LONG = [[i, 900] for i in range(64)]


@pytest.mark.gpu
def test_gpu_budget_exits_and_reentries(built, monkeypatch):
    """64 x 900 compressions, 2.35e6 instructions a lane: the loop leaves on the core's
    budget (2^20) twice and comes back through R and the loop's head"""
    rets, st, cnt, h = _parity(monkeypatch, "long", W.blake3_wasm(), LONG)
    assert int(min(cnt)) > 2 << 20 and all(int(s) == 0 for s in st)


@pytest.mark.gpu
def test_gpu_lanes_leave_on_every_early_trip(built, monkeypatch):
    rows = [[i, 1 + i % 7] for i in range(65)]
    _parity(monkeypatch, "div", W.blake3_wasm(), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [0, 1, 2])
def test_gpu_few_trips(built, monkeypatch, iters):
    rows = [[i, iters] for i in range(65)]
    _parity(monkeypatch, ("few", iters), W.blake3_wasm(), rows)


@pytest.mark.gpu
def test_gpu_chain_module(built, monkeypatch):
    rows = [[(i * 2654435761 + 7) & 0xFFFFFFFF, i % 5] for i in range(65)]
    _parity(monkeypatch, "chain", chain_module(), rows)


@pytest.mark.gpu
def test_gpu_lanes_wait_at_other_pcs(built, monkeypatch):
    """per-instance calls: even lanes run(i, 5), odd lanes the blake3 export on 100 bytes --
    while a group is in the chain loop the others wait at their own pcs (LOW, OTHER set)"""
    from wasmedge_amd import batch
    wasm, n = W.blake3_wasm(), 66
    func_of = [i % 2 for i in range(n)]
    rows = [[(i, I32), (5, I32)] if i % 2 == 0 else [(0, I32), (100, I32), (512, I32)] for i in range(n)]
    m = O.Module(wasm)
    ref = _ref("calls", lambda: [m.run(("run", "blake3")[func_of[i]], [v for v, _ in rows[i]]) for i in range(n)])

    def run():
        ctx = batch.BatchContext(wasm, n, device=0)
        try:
            rets, st, cnt = ctx.execute_calls(["run", "blake3"], func_of, rows)
            return rets, st, cnt, ctx.memory_hash()
        finally:
            ctx.close()

    on = _on_off(monkeypatch, run)
    assert compare(ref, *on, None, exact=True) == []


@pytest.mark.gpu
def test_gpu_max_steps_inside_the_third_budget(built, monkeypatch):
    """(on against off only: interruption is coarse and the oracle does not model it)"""
    run = lambda: gpu_run(W.blake3_wasm(), "run", LONG, [I32, I32], [I32], max_steps=2200000)
    rets, st, cnt, h = _on_off(monkeypatch, run)
    assert all(int(s) != 0 for s in st) and int(min(cnt)) >= 2200000


@pytest.mark.gpu
def test_gpu_gas_limit_falls_mid_loop(built, monkeypatch):
    """a metered context: lanes with four or more compressions run out of gas in the loop"""
    wasm, limit = W.blake3_wasm(), 10000
    rows = [[i, 1 + i % 7] for i in range(65)]
    m = O.Module(wasm)
    ref = _ref("gas", lambda: [O.Instance(m, cost_limit=limit).invoke("run", r) for r in rows])
    assert len({r[0] for r in ref}) == 2
    on = _on_off(monkeypatch, lambda: gpu_run(wasm, "run", rows, [I32, I32], [I32], cost_limit=limit))
    assert compare(ref, *on, [I32]) == []
