"""Instance-snapshot timings (WasmEdge_BatchSnapshotCreate / Restore, DESIGN.md "Instance
snapshots") at 64K instances, device-event time, median of 7 after 2 warm-ups, the compared
variants alternating in one process, with the spread (min, max) of every figure:

  * identity restore of the state a run left, beside a device-to-device copy of the same
    number of snapshot bytes and a timed BatchReset from the same state (the yardsticks);
  * forks (broadcast of instance 0, rotation within waves, random SrcOf) against the
    identity restore of the same snapshot;
  * end to end: Reset + Run(setup) + Run(step) against Restore + Run(step), wall clock,
    results and memory hashes bit-identical between the two ways.

Shapes: c2 (BLAKE3, small marks), c3_4k and c3_1m (quicksort of 4096 / 262144 i32, large
marks), granules 4 and 128 bytes.

    python tools/snapshot_probe.py [--instances 65536] [--shapes c2,c3_4k,c3_1m]
                                   [--out profiles/snapshot_probe.json]

--select measures the selective restore instead (WasmEdge_BatchSnapshotRestoreSelected /
RestoreSelectedDevice, DESIGN.md "Selective restore") on c2 and c3_4k, same method: the
identity restore(snap) as the yardstick, then `none`, `all`, whole waves kept for half of the
waves, `alternate`, 10% of the lanes restored from themselves and the same 10% from random
sources, each with the bytes of memory 0 its plan reads and writes; and, on c2, the wall clock
of the 10% restore from a host map against the same map already on the device. One JSON line,
written to profiles/snapshot_select_<first 8 digits of the source hash>.json.

    python tools/snapshot_probe.py --select [--instances 65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wasmedge_amd import batch, workloads   # noqa: E402

I32 = batch.I32
HBM_PEAK = 8e12   # bytes/s (MI355X)
SHAPES = {
    "c2": (workloads.blake3_wasm, "run", lambda ids: np.stack([ids, np.full_like(ids, 4)], 1), {}),
    "c3_4k": (workloads.qsort_wasm, "sort", lambda ids: np.stack([ids, np.full_like(ids, 4096)], 1),
              {"max_memory_page": 17}),
    "c3_1m": (workloads.qsort_wasm, "sort", lambda ids: np.stack([ids, np.full_like(ids, 262144)], 1),
              {"max_memory_page": 17}),
}


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def alternate(fns, reps=7, warm=2):
    """fns: {name: callable returning seconds}; one of each per round"""
    out = {k: [] for k in fns}
    for r in range(warm + reps):
        for k, f in fns.items():
            t = f()
            if r >= warm:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


KEEP = batch.KEEP


def select_maps(n):
    """the measured maps, uint32 [n] with KEEP for a kept lane"""
    ids = np.arange(n, dtype=np.uint32)
    rng = np.random.RandomState(9)
    tenth = rng.rand(n) < 0.1
    return {"none": ids.copy(), "all": np.full(n, KEEP, np.uint32),
            "half_waves": np.where((ids >> 6) & 1, np.uint32(KEEP), ids),
            "alternate": np.where(ids & 1, np.uint32(KEEP), ids),
            "tenth_self": np.where(tenth, ids, np.uint32(KEEP)),
            "tenth_random": np.where(tenth, rng.randint(0, n, n).astype(np.uint32), np.uint32(KEEP))}


def implied_bytes(m, wave_bytes, granule):
    """Bytes of memory 0 the plan of map m reads and writes, wave by wave (snapshot_plan.h
    plan_restore and the kernels' paths). wave_bytes: what a wave's marks bound, the same for
    every wave of these shapes and the same now as at the capture, taken from the snapshot's
    size. A wave without kept lanes reads and writes its rows once. A mixed wave whose
    restored lanes share a source wave reads that wave's rows whole, otherwise each restored
    lane's own; it reads the live tiles and writes them whole where a 16-byte piece spans
    lanes (granules below 16 bytes), and writes the restored lanes' pieces alone otherwise."""
    n = len(m)
    rd = wr = 0
    for w in range(0, n, 64):
        lanes = m[w:w + 64]
        rest = lanes[lanes != KEEP]
        if len(rest) == 0:
            continue
        share = len(rest) / len(lanes)
        if len(rest) == len(lanes):
            rd += wave_bytes
            wr += wave_bytes
            continue
        one = len(set(int(x) >> 6 for x in rest)) == 1
        rd += wave_bytes if one else wave_bytes * share
        if granule < 16:
            rd += wave_bytes
            wr += wave_bytes
        else:
            wr += wave_bytes * share
    return int(rd), int(wr)


def select_probe(n):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "wasmedge_amd", "csrc"))
    import srchash
    maps = select_maps(n)
    ids = np.arange(n, dtype=np.int64)
    rows = []
    plan = None
    for shape in ("c2", "c3_4k"):
        make, func, build, kw = SHAPES[shape]
        wasm = make()
        for granule in (4, 128):
            ctx = batch.BatchContext(wasm, n, device=0, memory_granule=granule, **kw)
            _, st, _ = ctx.execute(func, batch.make_values(build(ids), [I32, I32]), 1)
            assert not st.any()
            snap = ctx.snapshot()
            nwaves = (n + 63) // 64
            wave_bytes = snap.nbytes // nwaves   # (memory 0 beside the small whole buffers: an upper bound)
            tens = {k: torch.from_numpy(v.view(np.int32)).to("cuda:0") for k, v in maps.items()}
            fns = {"identity": lambda: ctx.restore(snap)}
            for k, v in maps.items():
                fns[k] = lambda v=v: ctx.restore_selected(snap, v.view(np.int32))[0]
            r = alternate(fns)
            row = {"shape": shape, "granule": granule, "instances": n, "snapshot_bytes": snap.nbytes,
                   "identity": r["identity"], "maps": {}}
            for k, v in maps.items():
                rd, wr = implied_bytes(v, wave_bytes, granule)
                row["maps"][k] = dict(r[k], read_bytes=rd, written_bytes=wr,
                                      Bps=(rd + wr) / r[k]["median_s"] if rd + wr else 0.0)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if shape == "c2" and granule == 4:
                # the plan: wall clock around the call (it ends in a synchronise), the host map
                # against the same map on the device, its producer long finished
                def wall(f):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    return time.perf_counter() - t0

                host = maps["tenth_random"].view(np.int32)
                plan = alternate({
                    "host_map": lambda: wall(lambda: ctx.restore_selected(snap, host)),
                    "device_map": lambda: wall(lambda: ctx.restore_tensor(snap, tens["tenth_random"]))})
                plan = {"shape": shape, "granule": granule, "map": "tenth_random", "wall_clock": plan}
                print(json.dumps(plan), flush=True)
            snap.close()
            ctx.close()
    out = os.path.join(ROOT, "profiles", "snapshot_select_%s.json" % srchash.source_hash()[:8])
    with open(out, "w") as fo:
        fo.write(json.dumps({"select": rows, "plan": plan, "source_hash": srchash.source_hash()}) + "\n")
    print("wrote " + out)


def main():
    import torch
    torch.zeros(1, device="cuda:0")   # (torch's HIP runtime finds its device first)
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--shapes", default="c2,c3_4k,c3_1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_probe.json"))
    ap.add_argument("--select", action="store_true", help="the selective restore (see above)")
    args = ap.parse_args()
    if args.select:
        select_probe(args.instances)
        return
    n = args.instances
    ids = np.arange(n, dtype=np.int64)
    rng = np.random.RandomState(3)
    forks = {"broadcast0": np.zeros(n, np.uint32),
             "rotate": ((ids & ~63) + ((ids & 63) + 1) % np.minimum(64, n - (ids & ~63))).astype(np.uint32),
             "random": rng.randint(0, n, n).astype(np.uint32)}
    rows = []
    for shape in args.shapes.split(","):
        make, func, build, kw = SHAPES[shape]
        wasm = make()
        for granule in (4, 128):
            ctx = batch.BatchContext(wasm, n, device=0, memory_granule=granule, **kw)
            vals = batch.make_values(build(ids), [I32, I32])
            _, st, _ = ctx.execute(func, vals, 1)
            assert not st.any()
            snap = ctx.snapshot()
            nbytes = snap.nbytes
            # the yardstick copy moves nbytes, through buffers of at most 4 GiB (a snapshot of
            # C3 at 1 MiB is 68 GB beside a 71 GB layout)
            chunk = min(nbytes, 4 << 30)
            a = torch.empty(chunk, dtype=torch.uint8, device="cuda:0")
            b = torch.empty_like(a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def copy():
                e0.record()
                for _ in range(nbytes // chunk):
                    b.copy_(a)
                if nbytes % chunk:
                    b[:nbytes % chunk].copy_(a[:nbytes % chunk])
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3

            def reset():
                t = ctx.reset()
                ctx.restore(snap)   # (back to the state the run left, untimed figure)
                return t

            r = alternate({"restore": lambda: ctx.restore(snap), "copy": copy, "reset": reset})
            bound = r["copy"]["median_s"] + r["reset"]["median_s"]
            margin = (r["copy"]["max_s"] - r["copy"]["min_s"]) + (r["reset"]["max_s"] - r["reset"]["min_s"])
            row = {"shape": shape, "granule": granule, "instances": n, "snapshot_bytes": nbytes,
                   "restore": r["restore"], "copy": r["copy"], "reset": r["reset"],
                   "copy_plus_reset_s": bound, "yardstick_spread_s": margin,
                   "restore_within_bound": r["restore"]["median_s"] <= bound + margin,
                   "restore_kernel_Bps": 2 * nbytes / r["restore"]["median_s"],
                   "restore_kernel_hbm_share": 2 * nbytes / r["restore"]["median_s"] / HBM_PEAK}
            f = alternate(dict({"identity": lambda: ctx.restore(snap)},
                               **{k: (lambda v=v: ctx.restore(snap, src_of=v)) for k, v in forks.items()}))
            row["fork"] = f
            row["fork_ratio"] = {k: f[k]["median_s"] / f["identity"]["median_s"] for k in forks}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del a, b
            snap.close()
            ctx.close()
    # end to end: C3's fill-and-sort of 4096 i32 as the setup, a 64-element sort as the step
    wasm = workloads.qsort_wasm()
    ctx = batch.BatchContext(wasm, n, device=0, max_memory_page=17)
    setup = batch.make_values(np.stack([ids, np.full_like(ids, 4096)], 1), [I32, I32])
    step = batch.make_values(np.stack([ids + 7, np.full_like(ids, 64)], 1), [I32, I32])

    def replay():
        t0 = time.perf_counter()
        ctx.reset(timed=False)
        ctx.execute("sort", setup, 1)
        out = ctx.execute("sort", step, 1)
        return time.perf_counter() - t0, out, ctx.memory_hash()

    replay()
    ctx.reset()
    ctx.execute("sort", setup, 1)
    snap = ctx.snapshot()

    def forked():
        t0 = time.perf_counter()
        ctx.restore(snap, timed=False)
        out = ctx.execute("sort", step, 1)
        return time.perf_counter() - t0, out, ctx.memory_hash()

    ta, tb = [], []
    for k in range(9):
        sa, oa, ha = replay()
        sb, ob, hb = forked()
        assert (ha == hb).all() and all((x == y).all() for x, y in zip(oa[1:], ob[1:])) and \
            (batch.ret_ints(oa[0]) == batch.ret_ints(ob[0])).all()
        if k >= 2:
            ta.append(sa)
            tb.append(sb)
    e2e = {"pair": "C3 sort(4096) as setup, sort(64) as step", "instances": n,
           "reset_setup_step": stats(ta), "restore_step": stats(tb),
           "speedup": statistics.median(ta) / statistics.median(tb), "bit_identical": True}
    print(json.dumps(e2e), flush=True)
    with open(args.out, "w") as fo:
        json.dump({"identity_and_fork": rows, "end_to_end": e2e,
                   "not_measured": [s for s in SHAPES if s not in args.shapes.split(",")]}, fo, indent=1)


if __name__ == "__main__":
    main()
