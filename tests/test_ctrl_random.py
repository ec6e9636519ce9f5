"""Random structured control-flow modules (tests/ctrl_cases.py), exact on every engine.

The suite pins control flow by hand-written modules only; every random generator it had
emits (local.set $d (op ..)) statements inside one fixed skeleton. These modules hold what
that skeleton never does: values (of 1, 2 and 4 cells) that live on the operand stack across
labels, blocks / loops / ifs with parameters and results, br / br_if / br_table that carry
values and unwind others at depths 0..3+, loops re-entered with new parameters and left from
two blocks inside, returns over junk, dead code after every kind of unconditional exit,
labels that only dead code or nothing reaches, stale local reads, producers that may and may
not be retargeted, runs of folded instructions of up to 300 (255 and 256 pending included)
before labels, loop heads and between a branch and its target, direct, indirect and
recursive calls in divergent arms, and traps under lane conditions. Everything is compared
with the oracle bit for bit, the instruction count of every instance included: one wrong
count correction on one edge shows as a count difference.

Every run is bounded: the generator terminates by construction (ctrl_cases' docstring), the
oracle runs under a gas limit that no row may reach, and every emulator and device run gets
max_steps = MAX_STEPS = 4 x ORACLE_MAX_COUNT, so that a scheduling bug shows as a status
mismatch (Interrupted) and not as a hang.

CPU: the generator's conditions measured on the oracle (conditions on the inputs: if one
fails, the generator changes, not the bound), the emulator against the oracle, assembly of
every module for gfx950 in the three flavours at three granules, and the count-only twin.
GPU: all seven engines of test_float_random, granules 4 and 128, WB_FWD_COUNT / WB_FOLD /
WB_INLINE off, partial waves of 8 and 65 instances, and the tail-call set on the three
engines of test_tailcall."""
import functools
import time

import pytest

import ctrl_cases as C
import oracle_py as O
from helpers import compare, emu_run, jit_check
from test_float_random import ENGINES, JIT_FLAVOURS
from wasmedge_amd.wat import assemble

I32, I64 = 0x7F, 0x7E
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7]
TAIL_SEEDS = [0, 1, 2]
# The oracle's step bound for the committed seeds: the largest instruction count of any row
# (8,858 in SEEDS, at seed 0; 11,545 in TAIL_SEEDS, at seed 1; asserted in _ref). Every run
# gets four times as many steps.
ORACLE_MAX_COUNT = 11545
MAX_STEPS = 4 * ORACLE_MAX_COUNT
GEN_CPU_SECONDS = 5.0      # generating and assembling one module; it takes about 0.05 s
COST_LIMIT_EXCEEDED = 0x03

ROWS = [[(i * 2654435761 + 12345) & 0xFFFFFFFF] for i in range(256)]   # (test_jit.ROWS)


@functools.lru_cache(maxsize=None)
def _wasm(seed, tail=False):
    t0 = time.process_time()
    wasm = C.ctrl_module(seed, tail)
    took = time.process_time() - t0
    assert took < GEN_CPU_SECONDS, "generating seed %d took %.1f s" % (seed, took)
    return wasm


@functools.lru_cache(maxsize=None)
def _ref(seed, tail=False):
    """the oracle's (code, values, count, memory hash) per row, computed once and shared;
    under a gas limit of MAX_STEPS unit costs, so that a module that did not terminate would
    fail here, loudly, instead of hanging"""
    m = O.Module(_wasm(seed, tail), tail_call=tail)
    rows = []
    for r in ROWS:
        row = O.Instance(m, cost_limit=MAX_STEPS).invoke("run", r)
        assert row[0] != COST_LIMIT_EXCEEDED and row[2] <= ORACLE_MAX_COUNT, (seed, tail, r, row)
        rows.append(row)
    return tuple(rows)


# ---------------------------------------------------------------- the generator's conditions
@functools.lru_cache(maxsize=None)
def _arms(seed):
    """per br_table of the module: (entries before the default, the indices that rows took)"""
    m = O.Module(_wasm(seed))
    n = C.tables(seed)
    taken = [set() for _ in n]
    for r in ROWS:
        mem = m.run_with_memory("run", r)[3]
        for j in range(len(n)):
            taken[j] |= {k for k in range(16) if mem[C.ARMS + 16 * j + k]}
    return list(zip(n, taken))


def stats_text():
    """the oracle-side statistics of the seed set (recorded in DESIGN.md "Parity tests")"""
    lines = ["seed | bytes | counts (distinct) | rows finishing | traps by code | br_tables (arms)"]
    for s in SEEDS:
        ref = _ref(s)
        codes = [x[0] for x in ref]
        cnts = [x[2] for x in ref]
        lines.append("%d | %d | %d-%d (%d) | %d | %s | %d (%d)" % (
            s, len(_wasm(s)), min(cnts), max(cnts), len(set(cnts)), codes.count(0),
            " ".join("%#x:%d" % (c, codes.count(c)) for c in sorted(set(codes)) if c),
            len(_arms(s)), sum(n + 1 for n, _ in _arms(s))))
    codes = [x[0] for s in SEEDS for x in _ref(s)]
    lines.append("pooled: %.1f%% of the rows trap; largest count %d" % (
        100.0 * sum(c != 0 for c in codes) / len(codes), max(x[2] for s in SEEDS for x in _ref(s))))
    return "\n".join(lines)


def test_generator_conditions():
    print(stats_text())
    missing = [t for t in C.REQUIRED if t not in C.constructs(SEEDS)]
    assert not missing, missing
    missing = [t for t in C.REQUIRED_TAIL if t not in C.constructs(TAIL_SEEDS, tail=True)]
    assert not missing, missing
    codes = []
    for s in SEEDS:
        ref = _ref(s)
        assert len({x[2] for x in ref}) >= 8, s                     # the lanes really diverge
        assert sum(x[0] == 0 for x in ref) * 2 >= len(ROWS), s      # at least half the rows finish
        codes += [x[0] for x in ref]
        for j, (n, taken) in enumerate(_arms(s)):                   # every arm, the default included
            assert {min(k, n) for k in taken} == set(range(n + 1)), (s, j, n, sorted(taken))
    assert 0.02 <= sum(c != 0 for c in codes) / len(codes) <= 0.30
    assert set(codes) == C.TRAP_CODES | {0}, sorted(set(codes))
    for s in TAIL_SEEDS:
        ref = _ref(s, True)
        assert len({x[2] for x in ref}) >= 8 and sum(x[0] == 0 for x in ref) * 2 >= len(ROWS), s


# ---------------------------------------------------------------- emulator against the oracle
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
def test_emulator_exact(built, tail):
    for s in TAIL_SEEDS if tail else SEEDS:
        got = emu_run(_wasm(s, tail), "run", ROWS, [I32], [I64], max_steps=MAX_STEPS, tail_call=tail)
        assert compare(_ref(s, tail), *got, [I64], exact=True) == [], s


# ---------------------------------------------------------------- assembly
@pytest.mark.parametrize("glog", [0, 2, 5])
def test_modules_assemble(built, glog):
    """every module assembles at every granule in the plain, SIMT and trip flavours, and has
    compiled runs"""
    for s in SEEDS:
        n, ins, text = jit_check(_wasm(s), glog, dump=("plain", "simt", "trip"))
        print("seed %d granule log %d: %d runs, %d instructions" % (s, glog, n, ins))
        assert n > 0 and ins > 0 and all(text[k] for k in ("plain", "simt", "trip")), s


# ---------------------------------------------------------------- the count-only twin
def test_count_only_twin():
    """The same modules without their nop / drop / select runs (ctrl_module(runs=False)) return
    the same value and status in every row, and fewer or as many instructions: the runs change
    counts only, so a count mismatch on the device points at the count corrections."""
    for s in SEEDS:
        twin = O.Module(C.ctrl_module(s, runs=False))
        assert len(twin.wasm) < len(_wasm(s))
        for r, ref in zip(ROWS, _ref(s)):
            code, vals, cnt, _ = twin.run("run", r)
            assert (code, vals) == (ref[0], ref[1]) and cnt <= ref[2], (s, r)


# ---------------------------------------------------------------- what the modules found
# A taken branch adds its count correction, which is negative where the branch skips folded
# instructions that the count of the instruction at its target includes. Within the first
# instructions of a run that carries the count below zero for a moment; the step limit,
# compared unsigned, then ended the instance with Interrupted (seed 4, whose br_if skips 255
# nops 90 instructions into run).
SKIP = assemble("(module (func (export \"run\") (param $s i32) (result i64)\n block local.get $s i32.const 1 i32.and "
                "br_if 0\n" + "nop " * 255 + "end\n local.get $s i64.extend_i32_u))")
SKIP_ROWS = [[k] for k in range(65)]


def _skip_ref():
    m = O.Module(SKIP)
    ref = [m.run("run", r) for r in SKIP_ROWS]
    assert ref[0][2] - ref[1][2] == 255 and ref[1][2] < 16     # (the taken branch skips the nops)
    return ref


def test_step_limit_after_a_negative_correction(built):
    got = emu_run(SKIP, "run", SKIP_ROWS, [I32], [I64], max_steps=1000)
    assert compare(_skip_ref(), *got, [I64], exact=True) == []


# ---------------------------------------------------------------- GPU
KNOBS = ("WB_SIMT", "WB_TRIP", "WB_JIT", "WB_VFRAME", "WB_THREADED", "WB_HBMFRAME", "WB_FOLD", "WB_FWD",
         "WB_FWD_COUNT", "WB_INLINE", "WB_TC_TAIL", "WB_NANOBS")
TAIL_ENGINES = {"compiled": {}, "core": {"WB_JIT": "0"}, "step": {"WB_JIT": "0", "WB_TC_TAIL": "0"}}


def _cases():
    out = [pytest.param(ENGINES[e], 0, 256, False, e in JIT_FLAVOURS, id=e) for e in ENGINES]
    for e in ("simt", "trip"):
        for g in (4, 128):
            out.append(pytest.param(ENGINES[e], g, 256, False, True, id="%s-granule%d" % (e, g)))
    for k in ("WB_FWD_COUNT", "WB_FOLD", "WB_INLINE"):
        out.append(pytest.param(dict(ENGINES["simt"], **{k: "0"}), 0, 256, False, True, id="simt-%s0" % k[3:].lower()))
    for e in ("simt", "interp"):
        for n in (8, 65):     # partial waves: divergence bookkeeping with inactive lanes
            out.append(pytest.param(ENGINES[e], 0, n, False, e in JIT_FLAVOURS, id="%s-%drows" % (e, n)))
    for e in TAIL_ENGINES:
        out.append(pytest.param(TAIL_ENGINES[e], 0, 256, True, e == "compiled", id="tail-" + e))
    return out


def gpu_case(granule, n, tail, seeds=None):
    """run() on one BatchContext per seed, through the C ABI; (differences, compiled runs)"""
    from wasmedge_amd import batch
    bad, runs = [], 0
    for s in seeds or (TAIL_SEEDS if tail else SEEDS):
        ctx = batch.BatchContext(_wasm(s, tail), n, memory_granule=granule, max_steps=MAX_STEPS, tail_call=tail)
        try:
            runs += ctx.compiled_runs()
            rets, st, cnt = ctx.execute("run", batch.make_values(ROWS[:n], [I32]), 1)
            h = ctx.memory_hash()
            ints = batch.ret_ints(rets)
            rows = [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(n)]
            bad += [(s,) + b for b in compare(_ref(s, tail)[:n], rows, st, cnt, h, [I64], exact=True)]
        finally:
            ctx.close()
    return bad, runs


def set_engine(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("env,granule,n,tail,jit", _cases())
def test_gpu_ctrl_random(built, monkeypatch, env, granule, n, tail, jit):
    set_engine(monkeypatch, env)
    bad, runs = gpu_case(granule, n, tail)
    assert bad == [], "%d rows differ, the first: %s" % (len({(b[0], b[1]) for b in bad}), bad[:6])
    if jit:
        assert runs > 0


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["simt", "trip", "interp", "step"])
def test_gpu_step_limit_after_a_negative_correction(built, monkeypatch, engine):
    from helpers import gpu_run
    set_engine(monkeypatch, ENGINES[engine])
    got = gpu_run(SKIP, "run", SKIP_ROWS, [I32], [I64], max_steps=1000)
    assert compare(_skip_ref(), *got, [I64], exact=True) == []
