"""Timings of snapshots that hold a suspended invocation (WasmEdge_BatchSnapshotCreateSuspended,
DESIGN.md "Snapshots of suspended runs") at 64K instances, median of 7 after 2 warm-ups, the
compared variants alternating in one process, with the spread (min, max) of every figure:

  * capture and identity restore of an invocation snapshot beside the plain snapshot's of the
    same state and a device-to-device copy (torch) of the bytes the invocation adds;
  * forks (broadcast of the deepest instance, random SrcOf) against the identity restore;
  * bytes held with and without the invocation, and the call-stack bytes against the whole
    buffer's.

Restores and the copy are device-event times. A capture has no device-time output, so both
captures are wall clock (perf_counter around the call, which ends with a stream
synchronisation), and the copy is given both ways.

States: c1 -- C1's divergent fib(20 + id mod 11) cut after two slices of 400,000 instructions (shallow: the
call stack stays in the LDS slots, no HBM rows); sum -- sum(1500 + id mod 64) by plain
recursion cut after 8,000 instructions, about 1000 levels and 2000 call-stack cells down.

    python tools/suspended_probe.py [--instances 65536] [--out profiles/suspended_probe.json]
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

from wasmedge_amd import batch   # noqa: E402
from wasmedge_amd.wat import assemble   # noqa: E402

I32 = batch.I32
SUM = r"""
(module
  (func $sum (export "sum") (param $n i32) (result i32)
    (if (result i32) (i32.eqz (local.get $n))
      (then (i32.const 0))
      (else (i32.add (local.get $n) (call $sum (i32.sub (local.get $n) (i32.const 1))))))))
"""
STACK_CELLS = 4096   # CallStackCells' default: the depth of the whole buffer while it has not grown


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def alternate(fns, reps=7, warm=2):
    out = {k: [] for k in fns}
    for r in range(warm + reps):
        for k, f in fns.items():
            t = f()
            if r >= warm:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


def main():
    import torch
    torch.zeros(1, device="cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suspended_probe.json"))
    args = ap.parse_args()
    n = args.instances
    nw = (n + 63) // 64
    ids = np.arange(n, dtype=np.int64)
    fib = open(os.path.join(ROOT, "tests", "golden", "fibonacci.wasm"), "rb").read()
    states = {"c1": (fib, "fib", (20 + ids % 11)[:, None], 400000, 2),
              "sum": (assemble(SUM), "sum", (1500 + ids % 64)[:, None], 8000, 1)}
    rng = np.random.RandomState(3)
    rows = []
    for name, (wasm, func, argv, s, slices) in states.items():
        ctx = batch.BatchContext(wasm, n, device=0, resumable=True, max_steps=s)
        ctx.set_args(func, batch.make_values(argv, [I32]))
        ctx.run()
        for k in range(2, slices + 1):
            ctx.resume(k * s)
        nsusp = ctx.suspended()
        _, st, cnt = ctx.results(1)
        assert nsusp > 0
        plain, inv = ctx.snapshot(), ctx.snapshot(invocation=True)
        assert inv.suspended == nsusp
        extra = inv.nbytes - plain.nbytes
        a = torch.empty(extra, dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy_dev():
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        def copy_wall():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.copy_(a)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def capture(invocation):
            ctx.restore(inv)   # (a live invocation again after the plain restores; untimed)
            t0 = time.perf_counter()
            sn = ctx.snapshot(invocation=invocation)
            t = time.perf_counter() - t0
            sn.close()
            return t

        cap = alternate({"invocation": lambda: capture(True), "plain": lambda: capture(False), "copy_wall": copy_wall})
        res = alternate({"invocation": lambda: ctx.restore(inv), "plain": lambda: ctx.restore(plain),
                         "copy": copy_dev})
        deepest = int(np.argmax(np.where(st == 0x07, argv[:, 0], -1)))
        forks = {"broadcast": np.full(n, deepest, np.uint32), "random": rng.randint(0, n, n).astype(np.uint32)}
        fk = alternate(dict({"identity": lambda: ctx.restore(inv)},
                            **{k: (lambda v=v: ctx.restore(inv, src_of=v)) for k, v in forks.items()}))
        # a restored batch still ends as the uninterrupted one would: one spot check per state
        ctx.restore(inv)
        k = slices
        while ctx.suspended() and k < slices + 3:
            k += 1
            ctx.resume(k * s)
        row = {"state": name, "instances": n, "slice": s, "slices_before_capture": slices, "suspended": nsusp,
               "bytes_plain": plain.nbytes, "bytes_invocation": inv.nbytes, "bytes_extra": extra,
               "whole_stack_bytes": nw * STACK_CELLS * 256,
               "capture_wall": cap, "restore": res, "fork": fk,
               "capture_extra_s": cap["invocation"]["median_s"] - cap["plain"]["median_s"],
               "restore_extra_s": res["invocation"]["median_s"] - res["plain"]["median_s"],
               "fork_ratio": {k: fk[k]["median_s"] / fk["identity"]["median_s"] for k in forks}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del a, b
        plain.close()
        inv.close()
        ctx.close()
    # both states have the same frame-save rows and per-instance arrays (the LDS share fixes
    # frame cells + LDS stack slots per wave; one result cell each), so the difference of what
    # the invocation adds is the packed call-stack rows of `sum` (c1 holds none)
    by = {r["state"]: r for r in rows}
    summary = {}
    if "c1" in by and "sum" in by:
        packed = by["sum"]["bytes_extra"] - by["c1"]["bytes_extra"]
        summary = {"sum_packed_stack_bytes": packed, "whole_stack_bytes": by["sum"]["whole_stack_bytes"],
                   "saved_bytes": by["sum"]["whole_stack_bytes"] - packed}
        print(json.dumps(summary), flush=True)
    with open(args.out, "w") as fo:
        json.dump({"states": rows, "stack": summary}, fo, indent=1)


if __name__ == "__main__":
    main()
