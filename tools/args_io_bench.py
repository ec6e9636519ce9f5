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

--per-instance times the per-instance staging instead (DESIGN.md "Device-resident per-instance
calls"): a call vector cycling over three functions of 1, 4 and 8 i64 parameters and 1, 4 and
1 results, WasmEdge_BatchSetCalls + BatchResults against WasmEdge_BatchSetCallsDevice +
BatchCallsResultsDevice, by the same method (tool "calls_io_bench" in the JSON line).
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


CALL_FUNCS = ((1, 1), (4, 4), (8, 1))   # (parameters, results) of the vector's functions


def per_instance(torch, args):
    """The per-instance pair: instance i calls CALL_FUNCS[i % 3]."""
    n, L = args.instances, batch.lib()
    rng = np.random.default_rng(2)
    funcs = ["p%dr%d" % pr for pr in CALL_FUNCS]
    wasm = assemble("(module %s)" % " ".join(
        '(func (export "p%dr%d") %s (result %s) %s)'
        % (p, r, " ".join(["(param i64)"] * p), " ".join(["i64"] * r),
           " ".join("(i64.add (local.get %d) (i64.const %d))" % (k % p, k) for k in range(r)))
        for p, r in CALL_FUNCS))
    ctx = batch.BatchContext(wasm, n, device=0)

    def ok(r):
        assert r.Code == 0, (r.Code, L.WasmEdge_BatchGetLastError(ctx._h))

    try:
        pmax, rmax = max(p for p, _ in CALL_FUNCS), max(r for _, r in CALL_FUNCS)
        fo = (np.arange(n) % len(CALL_FUNCS)).astype(np.uint32)
        plens = np.array([CALL_FUNCS[j][0] for j in fo], np.uint32)
        rows = rng.integers(0, 1 << 63, (n, pmax), dtype=np.uint64)
        vals = batch.make_values(rows, [batch.I64] * pmax)
        rets = np.zeros((n, rmax), batch.VALUE_DTYPE)
        lens, st, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        names, arr, tptrs, tlens, keep = batch.call_names(funcs, [[batch.I64] * p for p, _ in CALL_FUNCS])
        d_fo = torch.from_numpy(fo.view(np.int32)).to("cuda:0")
        d_rows = torch.from_numpy(rows.view(np.int64)).to("cuda:0")
        d_rets = torch.zeros((n, rmax), dtype=torch.int64, device="cuda:0")
        d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_st = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        d_cnt = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()

        def host_set():
            ok(L.WasmEdge_BatchSetCalls(ctx._h, arr, len(names), fo.ctypes.data, vals.ctypes.data, pmax,
                                        plens.ctypes.data))

        def host_get():   # (what ExecuteCalls reads: the result counts, then the rows)
            ok(L.WasmEdge_BatchGetReturnLens(ctx._h, lens.ctypes.data))
            ok(L.WasmEdge_BatchResults(ctx._h, rets.ctypes.data, rmax, st.ctypes.data, cnt.ctypes.data))

        def dev_set():
            ok(L.WasmEdge_BatchSetCallsDevice(ctx._h, arr, len(names), tptrs, tlens, d_fo.data_ptr(),
                                              d_rows.data_ptr(), pmax))

        def dev_get():
            ok(L.WasmEdge_BatchCallsResultsDevice(ctx._h, d_rets.data_ptr(), rmax, rmax, d_lens.data_ptr(),
                                                  d_st.data_ptr(), d_cnt.data_ptr()))

        host_set()
        ctx.run()
        t_hs = median_us(host_set, args.calls, args.warmup)
        t_hg = median_us(host_get, args.calls, args.warmup)
        dev_set()
        ctx.run()
        t_ds = median_us(dev_set, args.calls, args.warmup)
        t_dg = median_us(dev_get, args.calls, args.warmup)
        # both paths must have given the same rows
        assert np.array_equal(d_rets.cpu().numpy().view(np.uint64), rets["lo"]) and not st.any()
        assert np.array_equal(d_lens.cpu().numpy().view(np.uint32), lens)
        assert np.array_equal(d_st.cpu().numpy(), st)
        assert np.array_equal(d_cnt.cpu().numpy().view(np.uint64), cnt)
        # the host copy of the vector after a device staging, fetched on first need
        t0 = time.perf_counter()
        ok(L.WasmEdge_BatchGetReturnLens(ctx._h, lens.ctypes.data))
        t_fetch = round((time.perf_counter() - t0) * 1e6, 1)
    finally:
        ctx.close()
    print(json.dumps({"tool": "calls_io_bench", "instances": n, "calls": args.calls, "warmup": args.warmup,
                      "value_type": "i64", "statistic": "median wall-clock microseconds per call",
                      "functions": [{"params": p, "results": r} for p, r in CALL_FUNCS],
                      "host_set_calls_us": t_hs, "host_results_us": t_hg, "host_us": round(t_hs + t_hg, 1),
                      "device_set_calls_us": t_ds, "device_results_us": t_dg, "device_us": round(t_ds + t_dg, 1),
                      "mirror_fetch_once_us": t_fetch}))


def main():
    import torch
    # (a torch with a HIP runtime of its own has to find its device before the library does)
    torch.zeros(1, device="cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-instance", action="store_true")
    args = ap.parse_args()
    if args.per_instance:
        return per_instance(torch, args)
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
