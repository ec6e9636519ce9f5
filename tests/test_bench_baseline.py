"""bench.py's cpu_baseline leg on CPU: the oracle sample of each config workload must be
checked bit for bit against the batched results (here the host emulator's, standing in
for the GPU's), traps included, and yield the C3 roofline's bytes per instruction."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import helpers  # noqa: E402


def _fake_gpu(wasm, func, rows, ptypes, rtype, max_pages=0):
    rets, st, cnt, h = helpers.emu_run(wasm, func, [list(map(int, r)) for r in rows],
                                       ptypes, [rtype], max_pages=max_pages)
    ret = np.array([(r[0] if r else 0) & 0xFFFFFFFFFFFFFFFF for r in rets], np.uint64)
    return {"counts": cnt, "hashes": h, "status": st, "ret": ret, "ret32": rtype == 0x7F}


@pytest.mark.parametrize("name,n,elements", [("c3", 64, 512), ("c4", 200, 0), ("c2", 32, 0)])
def test_cpu_baseline_checks_sample(name, n, elements):
    import bench
    args = types.SimpleNamespace(iters=3, elements=elements)
    wasm, func, build_rows, ptypes, _desc, _extra = bench.workload(name, args)
    rows = build_rows(np.arange(n, dtype=np.int64))
    gpu = _fake_gpu(wasm, func, rows, [0x7F] * len(ptypes), 0x7F,
                    max_pages=17 if name == "c3" else 0)
    if name == "c4":
        assert (gpu["status"] != 0).any()   # the sample covers per-lane traps
    rec, bpi, (ld, stb) = bench.cpu_baseline(wasm, func, build_rows, ptypes, 0.5, 2, gpu, name.upper())
    assert rec["kind"] == "port" and rec["cores"] == 2 and rec["value"] > 0
    assert bpi > 0 and ld > 0 and stb >= 0 and abs(ld + stb - bpi) < 1e-9 * bpi
    if name in ("c2", "c3"):
        assert stb > 0   # (C4 only loads)
    # a wrong result for any sampled instance must fail the run loudly
    gpu["counts"] = gpu["counts"].copy()
    gpu["counts"][0] += 1
    with pytest.raises(SystemExit):
        bench.cpu_baseline(wasm, func, build_rows, ptypes, 0.5, 2, gpu, name.upper())


def test_check_engine_fails_on_silent_fallback(monkeypatch):
    """A bench line must not silently measure the threaded core after a compile failure
    (VERDICT r4 item 6): 0 compiled runs exits non-zero unless WB_JIT=0 asked for it."""
    import bench
    monkeypatch.delenv("WB_JIT", raising=False)
    bench.check_engine("c2", 12, "compiled-runs+simt/vgpr-frames")
    with pytest.raises(SystemExit) as e:
        bench.check_engine("c2", 0, "threaded-core (compiled runs failed)", "hiprtc: boom")
    assert "0 compiled runs" in str(e.value) and "hiprtc: boom" in str(e.value)
    monkeypatch.setenv("WB_JIT", "0")
    bench.check_engine("c2", 0, "threaded-core/vgpr-frames")


def test_vary_ids_are_fresh_permutations():
    """--vary-args: every step gives every instance another id (C5: another tile of the
    4096^2 image, a permutation of the 262,144 tiles)."""
    import bench
    ids = np.arange(262144, dtype=np.int64)
    seen = [ids]
    for k in range(3):
        v = bench.vary_ids(ids, k, "c5")
        assert sorted(v.tolist()) == ids.tolist()
        assert all((v != s).all() for s in seen)
        seen.append(v)
    v = bench.vary_ids(np.arange(65536, dtype=np.int64), 0, "c2")
    assert (v != np.arange(65536)).all() and v.max() < (1 << 30)


def test_dump_outputs_are_exact_float64(tmp_path, monkeypatch):
    """--dump-outputs: return values as (low, high) 32-bit halves, status and counts, all
    float64 and exact; a trapped instance's return value (undefined) is written as 0."""
    import bench
    from wasmedge_amd import batch
    rets = np.zeros((4, 1), batch.VALUE_DTYPE)
    rets["lo"][:, 0] = [7, (1 << 63) + 5, 0xDEADBEEF, 1 << 32]
    st = np.array([0, 0, 0x88, 0], np.uint8)
    cnt = np.array([1, 1 << 40, 3, 4], np.uint64)
    bench.dump_outputs(str(tmp_path / "d"), types.SimpleNamespace(rank=0, world=1), rets, st, cnt)
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("returns", "status", "counts")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["returns"].tolist() == [[7, 0], [5, 1 << 31], [0, 0], [0, 1]]
    assert got["status"].tolist() == [0, 0, 0x88, 0] and got["counts"].tolist() == [1, 1 << 40, 3, 4]
    # past the size cap: the same seeded sample of instances every time, with its index
    monkeypatch.setattr(bench, "DUMP_MAX_INSTANCES", 2)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), types.SimpleNamespace(rank=0, world=1), rets, st, cnt)
    idx = np.load(str(tmp_path / "s1" / "index.npy"))
    assert idx.shape == (2,) and np.array_equal(idx, np.load(str(tmp_path / "s2" / "index.npy")))
    assert np.array_equal(np.load(str(tmp_path / "s1" / "counts.npy")), got["counts"][idx.astype(int)])


def _bench(*argv):
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.gpu
def test_gpu_bench_plain_run_is_lean_and_full_keeps_every_leg(built, tmp_path):
    """A plain run times exactly --steps steps and prints the headline keys only; --full adds
    the CPU baseline (bit-exact check), checksum and rooflines; --dump-outputs writes the
    same arrays from run to run, equal to the oracle's for the same instances."""
    import oracle_py
    import bench
    small = ["--gpus", "1", "--instances", "192", "--iters", "3", "--steps", "2", "--warmup", "1"]
    a = _bench(*small, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*small, "--full", "--cpu-seconds", "0.4", "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "instr/s"
        assert line["higher_is_better"] is True and line["dtype"] == "i32" and line["metric"] == bench.METRIC
        assert abs(line["value"] - 192 * line["config"]["instrs_per_instance"] / (1e-3 * line["ms_per_step"])) \
            <= 1e-9 * line["value"]
    moved = ("cpu_baseline", "memory_checksum", "roofline", "hbm_roofline")
    assert not any(k in a for k in moved) and all(k in b for k in moved)
    got = {n: (np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy"))))
           for n in ("returns", "status", "counts")}
    for x, y in got.values():
        assert x.dtype == np.float64 and x.shape[0] == 192 and np.array_equal(x, y)
    wasm, func, build_rows, ptypes, _desc, _extra = bench.workload("c2", types.SimpleNamespace(iters=3))
    m = oracle_py.Module(wasm)
    for i, row in enumerate(build_rows(np.arange(192, dtype=np.int64)).tolist()):
        code, ref, rcnt, _ = m.run(func, row)
        assert (code, ref[0] & 0xFFFFFFFF, rcnt) == \
            (got["status"][0][i], got["returns"][0][i, 0], got["counts"][0][i]), i   # (C2 returns an i32)


def test_default_instances_are_the_metric_config():
    import bench
    assert bench.default_instances("c2") == 65536 and bench.default_instances("c3") == 65536
    assert bench.default_instances("c5") == 262144
