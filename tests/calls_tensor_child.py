"""Run by tests/test_calls_device.py in a process of its own: set_calls_tensor /
calls_results_tensor, the torch mirror of WasmEdge_BatchSetCallsDevice / CallsResultsDevice.
torch initialises its device BEFORE the first BatchContext exists -- a torch build with a HIP
runtime of its own finds no GPU when it starts second, and the test suite's process has long
created contexts. Prints one JSON line: whether the tensor path equals the host path on the
mixed vector at 130 instances, and whether each malformed tensor is refused.

    python tests/calls_tensor_child.py
"""
import json
import os
import sys

import numpy as np
import torch

torch.cuda.init()
torch.zeros(1, device="cuda:0")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_calls_device as T     # noqa: E402


def refused(fn):
    try:
        fn()
    except ValueError:
        return True
    return False


def main():
    n = T.N
    vec = T.mixed(n)
    ctx = T.calls_ctx(n)
    try:
        T.stage_host(ctx, vec)
        ctx.run()
        width = T.WIDEST_R + 1
        want, wl, st, cnt = T.read_host(ctx, width)
        hashes = ctx.memory_hash()
        ctx.reset()
        fo = torch.from_numpy(vec.fo().view(np.int32)).to("cuda:0")
        rows = torch.from_numpy(vec.slots().view(np.int64)).to("cuda:0")
        ctx.set_calls_tensor(vec.funcs, fo, rows, types=vec.types)
        ctx.run()
        # into tensors of the caller's, rows two slots wider than Width
        out = torch.full((n, width + 2), 0x5AA5, dtype=torch.int64, device="cuda:0")
        dl = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        dst = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda:0")
        dcnt = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
        r = ctx.calls_results_tensor(width, out=out, lens=dl, status=dst, counts=dcnt)
        got = out.cpu().numpy().view(np.uint64)
        # ... and into tensors the call allocates
        out2, l2, st2, cnt2 = ctx.calls_results_tensor(width)
        wrong = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
        res = {
            "values_equal": bool(np.array_equal(got[:, :width], want)),
            "padding_kept": bool((got[:, width:] == 0x5AA5).all()) and all(a is b for a, b in zip(r, (out, dl, dst, dcnt))),
            "lens_equal": bool(np.array_equal(dl.cpu().numpy().view(np.uint32), wl)),
            "status_equal": bool(np.array_equal(dst.cpu().numpy(), st)),
            "counts_equal": bool(np.array_equal(dcnt.cpu().numpy().view(np.uint64), cnt)),
            "memories_equal": bool(np.array_equal(ctx.memory_hash(), hashes)),
            "allocated_equal": tuple(out2.shape) == (n, width)
            and bool(np.array_equal(out2.cpu().numpy().view(np.uint64), want))
            and bool(np.array_equal(l2.cpu().numpy().view(np.uint32), wl))
            and bool(np.array_equal(st2.cpu().numpy(), st))
            and bool(np.array_equal(cnt2.cpu().numpy().view(np.uint64), cnt)),
            "refused": {
                "non_contiguous": refused(lambda: ctx.set_calls_tensor(vec.funcs, fo, wrong[:, :7])),
                "cpu": refused(lambda: ctx.set_calls_tensor(vec.funcs, fo, rows.cpu())),
                "dtype": refused(lambda: ctx.set_calls_tensor(vec.funcs, fo, rows.to(torch.float64))),
                "func_of_dtype": refused(lambda: ctx.set_calls_tensor(vec.funcs, fo.to(torch.int64), rows)),
                "out_non_contiguous": refused(lambda: ctx.calls_results_tensor(4, out=wrong[:, :7])),
                "out_cpu": refused(lambda: ctx.calls_results_tensor(4, out=wrong.cpu())),
                "lens_dtype": refused(lambda: ctx.calls_results_tensor(4, lens=dcnt)),
            },
        }
    finally:
        ctx.close()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
