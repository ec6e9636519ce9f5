"""Random float and SIMD modules (tests/float_cases.py), bit-exact on every flavour of the
compiled runs (wasmedge_amd/csrc/jit.cpp) and on every engine.

The hand-written matrices (scalar_cases, simd_cases) apply each op once to operands fresh
from memory and store the result at once: every operand is intact, every result is
observable, nothing aliases. The in-place NaN repair (Em::nan_fix) and the backward
dataflow that decides which results keep it (nan_observable, also the liveness behind the
WB_FOLD folds) can only go wrong elsewhere: where a destination aliases a source, where a
NaN flows through a chain or across a divergent branch, a loop back edge, a call, a
br_table or a trap, and where a run starts or ends with a NaN in flight between the core
and the C++ step. The random modules go there; everything is compared with the oracle bit
for bit (compare(..., exact=True)): return bits, status, instruction counts, the memory
hash of finished and trapped instances, and the globals through getters run afterwards on
the same instances.

CPU: the generator's own conditions measured on the oracle (NaN shares, trap shares and
codes, op coverage: conditions on the inputs -- if one fails the generator changes, not the
bound), the host emulator against the oracle, and every module assembled for gfx950 at
three granules, with the mnemonic families the float emitter can produce present and
0 < fixes(WB_NANOBS=1) < fixes(WB_NANOBS=0) in every module.
GPU: every engine and flavour with both op mixes, WB_NANOBS=0 on the three JIT flavours,
WB_FOLD=0 and WB_FWD=0, and memory granules 4 and 128 (a 16-byte access spans four
granules of 4 bytes) with and without trip mode."""
import functools
import re
import struct

import pytest

import float_cases as F
import oracle_py as O
from helpers import compare, emu_run, jit_check

I32, I64, V128 = 0x7F, 0x7E, 0x7B
# (three of them, 11, 20 and 15, are seeds at which the analysis once dropped a fix that was needed)
SEEDS = [0, 1, 2, 11, 20, 5, 6, 15]
ROWS = [[(i * 2654435761 + 12345) & 0xFFFFFFFF] for i in range(256)]   # (test_jit.ROWS)
MIXES = ["compiled", "mixed"]
GETTERS = [("g32", I32), ("g64", I64), ("gv", V128)]


@functools.lru_cache(maxsize=None)
def _wasm(mix, seed):
    return F.float_module(seed, mix)


@functools.lru_cache(maxsize=None)
def _ref(mix, seed):
    """The oracle's answers, computed once and shared: per row (code, values, count, memory
    hash) of run(), and per getter the values read afterwards on the same instance."""
    m = O.Module(_wasm(mix, seed))
    rows, getters = [], {g: [] for g, _ in GETTERS}
    for r in ROWS:
        inst = O.Instance(m)
        rows.append(inst.invoke("run", r))
        for g, _ in GETTERS:
            code, vals, _, _ = inst.invoke(g, [])
            assert code == 0
            getters[g].append(vals[0])
    return tuple(rows), getters


# ---------------------------------------------------------------- the generator's conditions
def _is_nan32(v):
    return (v & 0x7FFFFFFF) > 0x7F800000


def _is_nan64(v):
    return (v & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000


@functools.lru_cache(maxsize=None)
def _stats():
    """per (mix, seed): status codes of the rows, and (NaNs, values) of the final f32 and f64
    locals of the rows that finished"""
    out = {}
    for mix in MIXES:
        for s in SEEDS:
            m = O.Module(_wasm(mix, s))
            codes, n32, n64, k = [], 0, 0, 0
            for r in ROWS:
                code, _, _, mem = m.run_with_memory("run", r)
                codes.append(code)
                if code:
                    continue
                k += F.NLOC
                n32 += sum(_is_nan32(v) for v in struct.unpack_from("<4I", mem, F.FINAL_F32))
                n64 += sum(_is_nan64(v) for v in struct.unpack_from("<4Q", mem, F.FINAL_F64))
            out[mix, s] = (codes, n32, n64, k)
    return out


def stats_text():
    """the oracle-side statistics of the seed set (recorded in DESIGN.md "Parity tests")"""
    st = _stats()
    lines = []
    for mix in MIXES:
        per = [st[mix, s] for s in SEEDS]
        k = sum(p[3] for p in per)
        codes = [c for p in per for c in p[0]]
        lines.append("%s: f32 NaN %.1f%% (per seed %s), f64 NaN %.1f%% (per seed %s), status 0 per seed %s, "
                     "traps %.1f%% %s" % (
                         mix, 100.0 * sum(p[1] for p in per) / k, " ".join("%.0f" % (100.0 * p[1] / p[3]) for p in per),
                         100.0 * sum(p[2] for p in per) / k, " ".join("%.0f" % (100.0 * p[2] / p[3]) for p in per),
                         " ".join("%.0f" % (100.0 * p[0].count(0) / len(ROWS)) for p in per),
                         100.0 * sum(c != 0 for c in codes) / len(codes),
                         {hex(c): codes.count(c) for c in sorted(set(codes)) if c}))
    return "\n".join(lines)


@pytest.mark.parametrize("mix", MIXES)
def test_generator_conditions(mix):
    st = _stats()
    print(stats_text())
    per = [st[mix, s] for s in SEEDS]
    k = sum(p[3] for p in per)
    assert 0.05 <= sum(p[1] for p in per) / k <= 0.50       # f32 NaN share, pooled
    assert 0.05 <= sum(p[2] for p in per) / k <= 0.50       # f64 NaN share, pooled
    codes = []
    for s, (c, n32, n64, vals) in zip(SEEDS, per):
        assert 0 < n32 + n64 < 2 * vals, s                  # a NaN and a non-NaN final value
        assert c.count(0) * 2 >= len(ROWS), s               # at least half the rows finish
        codes += c
    assert sum(x != 0 for x in codes) >= 0.02 * len(codes)
    assert {0x84, 0x85, 0x86, 0x88} <= set(codes), sorted(set(codes))


def test_generator_names_every_op():
    wats = {mix: [F.float_wat(s, mix) for s in SEEDS] for mix in MIXES}
    assert not set(F.COMPILED_OPS) - F.ops_covered(wats["compiled"], F.COMPILED_OPS)
    both = F.COMPILED_OPS + F.MIXED_OPS
    assert not set(both) - F.ops_covered(wats["mixed"], both)
    # the compiled mix stays inside its list
    assert not F.ops_covered(wats["compiled"], F.MIXED_OPS)


# ---------------------------------------------------------------- emulator against the oracle
@pytest.mark.parametrize("mix", MIXES)
def test_emulator_exact(built, mix):
    for s in SEEDS:
        wasm = _wasm(mix, s)
        ref, _ = _ref(mix, s)
        got = emu_run(wasm, "run", ROWS, [I32], [I64])
        assert compare(ref, *got, [I64], exact=True) == [], s
        # the getters, on an instance of each side that has not run (an emulator run keeps no
        # state), and the globals a finished run leaves, through rung
        inst = O.Instance(O.Module(wasm))
        for g, t in GETTERS:
            got = emu_run(wasm, g, [[]], [], [t])
            assert compare([inst.invoke(g, [])], *got, [t], exact=True) == [], (s, g)
        m = O.Module(wasm)
        gref = [m.run("rung", r) for r in ROWS]
        got = emu_run(wasm, "rung", ROWS, [I32], [I64])
        assert compare(gref, *got, [I64], exact=True) == [], s


# ---------------------------------------------------------------- assembly, liveness
FAMILIES = [r"v_add_f32", r"v_sub_f32", r"v_mul_f32", r"v_add_f64", r"v_mul_f64", r"v_cmp_\w+_f32",
            r"v_cmp_\w+_f64", r"v_cvt_f64_i32", r"v_cvt_f32_u32", r"v_bfi_b32"]


@pytest.mark.parametrize("glog", [0, 2, 5])
def test_modules_assemble(built, monkeypatch, glog):
    """every module assembles at every granule, in every flavour; at granule log 0 the SIMT
    text of the compiled mix holds every float/vector mnemonic family, and the analysis drops
    some NaN fixes of every module and keeps others"""
    monkeypatch.setenv("WB_NANOBS", "1")
    simt = {}
    for mix in MIXES:
        for s in SEEDS:
            n, ins, text = jit_check(_wasm(mix, s), glog, dump=("plain", "simt", "trip"))
            assert n > 0 and ins > 0 and all(text[k] for k in ("plain", "simt", "trip")), (mix, s)
            simt[mix, s] = text["simt"]
    if glog:
        return
    pooled = "\n".join(simt["compiled", s] for s in SEEDS)
    missing = [f for f in FAMILIES if not re.search(f, pooled)]
    assert not missing, missing
    monkeypatch.setenv("WB_NANOBS", "0")
    for (mix, s), text in simt.items():
        on = text.count("v_cmp_u_f")
        off = jit_check(_wasm(mix, s), 0, dump="simt")[2].count("v_cmp_u_f")
        print("%s seed %d: NaN fixes %d of %d" % (mix, s, on, off))
        assert 0 < on < off, (mix, s, on, off)


# ---------------------------------------------------------------- GPU
# The three flavours of the compiled runs, then the engines without them. The default picks
# trip mode for these modules (wb_trip_choice), so "simt" turns it off, as tests/test_jit.py does.
ENGINES = {"simt": {"WB_TRIP": "0"}, "plain": {"WB_SIMT": "0"}, "trip": {"WB_TRIP": "1"},
           "interp": {"WB_JIT": "0"}, "ldsframe": {"WB_VFRAME": "0"}, "step": {"WB_THREADED": "0"},
           "hbmframe": {"WB_HBMFRAME": "1"}}
JIT_FLAVOURS = ("simt", "plain", "trip")


def _cases():
    out = []
    for e in ENGINES:
        for mix in MIXES:
            out.append(pytest.param(ENGINES[e], mix, 0, e in JIT_FLAVOURS, id="%s-%s" % (e, mix)))
    for e in JIT_FLAVOURS:
        for mix in MIXES:
            out.append(pytest.param(dict(ENGINES[e], WB_NANOBS="0"), mix, 0, True, id="%s-%s-nanobs0" % (e, mix)))
    out.append(pytest.param(dict(ENGINES["simt"], WB_FOLD="0"), "compiled", 0, True, id="simt-fold0"))
    out.append(pytest.param(dict(ENGINES["simt"], WB_FWD="0"), "compiled", 0, True, id="simt-fwd0"))
    for e in ("simt", "trip"):
        for g in (4, 128):
            out.append(pytest.param(ENGINES[e], "mixed", g, True, id="%s-mixed-granule%d" % (e, g)))
    return out


def gpu_case(env, mix, granule, seeds=SEEDS):
    """run() and then the three getters on one BatchContext per seed, through the C ABI;
    returns (differences, compiled runs)"""
    from wasmedge_amd import batch
    bad, runs = [], 0
    none = batch.make_values([[] for _ in ROWS], [])
    for s in seeds:
        wasm = _wasm(mix, s)
        ref, gref = _ref(mix, s)
        ctx = batch.BatchContext(wasm, len(ROWS), memory_granule=granule)
        try:
            runs += ctx.compiled_runs()
            rets, st, cnt = ctx.execute("run", batch.make_values(ROWS, [I32]), 1)
            h = ctx.memory_hash()
            ints = batch.ret_ints(rets)
            rows = [[int(x) for x in ints[i]] if st[i] == 0 else [] for i in range(len(ROWS))]
            bad += [(s,) + b for b in compare(ref, rows, st, cnt, h, [I64], exact=True)]
            # globals are observable after a trap too: every instance answers
            for g, _ in GETTERS:
                rets, gst, _ = ctx.execute(g, none, 1)
                ints = batch.ret_ints(rets)
                bad += [(s, i, g, gref[g][i], int(ints[i][0]), int(gst[i])) for i in range(len(ROWS))
                        if int(gst[i]) != 0 or int(ints[i][0]) != gref[g][i]]
        finally:
            ctx.close()
    return bad, runs


@pytest.mark.gpu
@pytest.mark.parametrize("env,mix,granule,jit", _cases())
def test_gpu_float_random(built, monkeypatch, env, mix, granule, jit):
    for k in ("WB_SIMT", "WB_TRIP", "WB_JIT", "WB_VFRAME", "WB_THREADED", "WB_HBMFRAME", "WB_NANOBS",
              "WB_FOLD", "WB_FWD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bad, runs = gpu_case(env, mix, granule)
    rows = {(b[0], b[1]) for b in bad}
    assert bad == [], "%d rows differ, the first: %s" % (len(rows), bad[:6])
    if jit:
        assert runs > 0
