"""What a slice boundary costs (WasmEdge_BatchResume, DESIGN.md "Resumable runs"): C2's
module (BLAKE3, 1000 chained compressions per instance, bench.py's default) at 64K instances
on a Resumable context, in one run and cut into 2, 8 and 32 equal slices of the instruction
count. Kernel time by HIP events (the library's own, summed over a variant's launches),
median of 7 after 2 warm-ups, the variants taken in turn in one process, min .. max beside
every median. The derived figure: (sliced - whole) / (slices - 1) per boundary. Every
variant's results are checked against the whole run's.

    python tools/resume_probe.py [--instances 65536] [--iters 1000] [--out profiles/resume_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wasmedge_amd import batch, workloads   # noqa: E402

I32 = batch.I32
SLICES = (1, 2, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_probe.json"))
    args = ap.parse_args()
    n = args.instances
    ids = np.arange(n, dtype=np.int64)
    vals = batch.make_values(np.stack([ids, np.full_like(ids, args.iters)], 1), [I32, I32])
    wasm = workloads.blake3_wasm()

    # the instruction count of one instance (uniform for C2) sizes the slices
    ctx = batch.BatchContext(wasm, n, device=0, resumable=True)
    want = ctx.execute("run", vals, 1)
    total = int(want[2].max())
    assert not want[1].any() and int(want[2].min()) == total
    engine = ctx.engine()
    ctx.close()

    ctxs = {}
    for k in SLICES:
        step = -(-total // k)
        ctxs[k] = (batch.BatchContext(wasm, n, device=0, resumable=True, max_steps=step if k > 1 else 0), step)
        ctxs[k][0].set_args("run", vals)

    def variant(k):
        ctx, step = ctxs[k]
        ctx.reset(timed=False)
        t = ctx.run()
        launches = 1
        while ctx.suspended():
            launches += 1
            assert launches <= k + 2
            t += ctx.resume(step * launches if launches < k else 0)
        return t, launches

    times = {k: [] for k in SLICES}
    launches = {}
    for r in range(9):
        for k in SLICES:
            t, launches[k] = variant(k)
            if r >= 2:
                times[k].append(t)
    for k in SLICES:   # (after the timed rounds: every variant ends as the whole run does)
        got = ctxs[k][0].results(1)
        assert all((a == b).all() for a, b in zip(want[1:], got[1:]))
        assert (batch.ret_ints(want[0]) == batch.ret_ints(got[0])).all()
        ctxs[k][0].close()
    whole = statistics.median(times[1])
    rows = []
    for k in SLICES:
        med = statistics.median(times[k])
        rows.append({"slices": k, "launches": launches[k], "kernel_s": med, "min_s": min(times[k]),
                     "max_s": max(times[k]),
                     "per_boundary_s": (med - whole) / (launches[k] - 1) if launches[k] > 1 else None})
        print(json.dumps(rows[-1]), flush=True)
    out = {"workload": "c2 (blake3 x %d)" % args.iters, "instances": n, "engine": engine,
           "instructions_per_instance": total, "variants": rows}
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
