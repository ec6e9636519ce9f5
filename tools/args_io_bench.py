"""What staging and reading a run costs per call, host path against device path (DESIGN.md
"Device-resident arguments and results"): WasmEdge_BatchSetArgs + BatchResults, which repack
N x P 32-byte values on one host thread and cross the host twice, against
WasmEdge_BatchSetArgsDevice + BatchResultsDevice on rows that stay on the device.

64K instances of a trivial module (the run itself is one launch of a few instructions and is
not timed), 1 and 8 i64 parameters, 1 and 4 i64 results. Each of the four entry points is
called directly through ctypes on buffers allocated once, so the figure is the library's, not
numpy's: wall clock around the call, which ends in a stream synchronise; the median of 20
calls after 3 warm-ups. Prints one JSON line (times in microseconds).

    python tools/args_io_bench.py [--instances 65536] [--calls 20] [--warmup 3]
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

from wasmedge_amd import batch          # noqa: E402
from wasmedge_amd.wat import assemble   # noqa: E402

PARAMS, RESULTS = (1, 8), (1, 4)


def module():
    """p<P>r<R>: P i64 parameters, R i64 results (parameter k mod P, plus k)"""
    funcs = []
    for p in PARAMS:
        for r in RESULTS:
            body = " ".join("(i64.add (local.get %d) (i64.const %d))" % (k % p, k) for k in range(r))
            funcs.append('(func (export "p%dr%d") %s (result %s) %s)'
                         % (p, r, " ".join(["(param i64)"] * p), " ".join(["i64"] * r), body))
    return assemble("(module %s)" % " ".join(funcs))


def median_us(fn, calls, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e6, 1)


def main():
    import torch
    # (a torch with a HIP runtime of its own has to find its device before the library does)
    torch.zeros(1, device="cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, L = args.instances, batch.lib()
    rng = np.random.default_rng(1)
    ctx = batch.BatchContext(module(), n, device=0)
    cases = []

    def ok(r):
        assert r.Code == 0, (r.Code, L.WasmEdge_BatchGetLastError(ctx._h))

    try:
        for p in PARAMS:
            for r in RESULTS:
                name = ("p%dr%d" % (p, r)).encode()
                fname = batch._String(len(name), name)
                rows = rng.integers(0, 1 << 63, (n, p), dtype=np.uint64)
                vals = batch.make_values(rows, [batch.I64] * p)
                rets = np.zeros((n, r), batch.VALUE_DTYPE)
                st, cnt = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
                types = np.array([batch.I64] * p, np.uint32)
                d_rows = torch.from_numpy(rows.view(np.int64)).to("cuda:0")
                d_rets = torch.zeros((n, r), dtype=torch.int64, device="cuda:0")
                d_st = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
                d_cnt = torch.zeros(n, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()

                def host_set():
                    ok(L.WasmEdge_BatchSetArgs(ctx._h, fname, vals.ctypes.data, p))

                def host_get():
                    ok(L.WasmEdge_BatchResults(ctx._h, rets.ctypes.data, r, st.ctypes.data, cnt.ctypes.data))

                def dev_set():
                    ok(L.WasmEdge_BatchSetArgsDevice(ctx._h, fname, types.ctypes.data, p, d_rows.data_ptr(), p))

                def dev_get():
                    ok(L.WasmEdge_BatchResultsDevice(ctx._h, d_rets.data_ptr(), r, r, d_st.data_ptr(),
                                                     d_cnt.data_ptr()))

                # one run per staging path, so that each Results reads rows of this function;
                # both paths must have given the same rows
                host_set()
                ctx.run()
                t_hs = median_us(host_set, args.calls, args.warmup)
                t_hg = median_us(host_get, args.calls, args.warmup)
                dev_set()
                ctx.run()
                t_ds = median_us(dev_set, args.calls, args.warmup)
                t_dg = median_us(dev_get, args.calls, args.warmup)
                assert np.array_equal(d_rets.cpu().numpy().view(np.uint64), rets["lo"]) and not st.any()
                assert np.array_equal(d_st.cpu().numpy(), st)
                assert np.array_equal(d_cnt.cpu().numpy().view(np.uint64), cnt)
                cases.append({"params": p, "results": r,
                              "host_set_args_us": t_hs, "host_results_us": t_hg, "host_us": round(t_hs + t_hg, 1),
                              "device_set_args_us": t_ds, "device_results_us": t_dg,
                              "device_us": round(t_ds + t_dg, 1)})
    finally:
        ctx.close()
    print(json.dumps({"tool": "args_io_bench", "instances": n, "calls": args.calls, "warmup": args.warmup,
                      "value_type": "i64", "statistic": "median wall-clock microseconds per call",
                      "cases": cases}))


if __name__ == "__main__":
    main()
