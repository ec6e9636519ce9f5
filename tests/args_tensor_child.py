"""Run by tests/test_args_device.py in a process of its own: set_args_tensor / results_tensor,
the torch mirror of WasmEdge_BatchSetArgsDevice / ResultsDevice. torch initialises its device
BEFORE the first BatchContext exists -- a torch build with a HIP runtime of its own finds no
GPU when it starts second, and the test suite's process has long created contexts. Prints one
JSON line: whether the tensor path equals the host path on mix at 130 instances, and whether
each malformed tensor is refused.

    python tests/args_tensor_child.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from wasmedge_amd import batch   # noqa: E402
import test_args_device as T     # noqa: E402


def refused(fn):
    try:
        fn()
    except ValueError:
        return True
    return False


def main():
    n = T.N
    slots = T.mix_slots(n, 77)
    ctx = batch.BatchContext(T.wasm(), n, device=0)
    try:
        T.stage_host(ctx, "mix", slots)
        ctx.run()
        want, st, cnt = T.read_host(ctx, "mix")
        ctx.reset()
        width = batch.slots_of(T.MIX_R)
        t = torch.from_numpy(slots.view(np.int64)).to("cuda:0")
        ctx.set_args_tensor("mix", T.MIX_P, t)
        ctx.run()
        # into tensors of the caller's, rows two slots wider than the results
        out = torch.full((n, width + 2), 0x5AA5, dtype=torch.int64, device="cuda:0")
        dst = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda:0")
        dcnt = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
        r = ctx.results_tensor(len(T.MIX_R), out=out, status=dst, counts=dcnt)
        got = out.cpu().numpy().view(np.uint64)
        # ... and into tensors the call allocates (the result types give the row width)
        out2, st2, cnt2 = ctx.results_tensor(T.MIX_R)
        wrong = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
        res = {
            "values_equal": bool(np.array_equal(got[:, :width], want)),
            "padding_kept": bool((got[:, width:] == 0x5AA5).all()) and r[0] is out and r[1] is dst and r[2] is dcnt,
            "status_equal": bool(np.array_equal(dst.cpu().numpy(), st)),
            "counts_equal": bool(np.array_equal(dcnt.cpu().numpy().view(np.uint64), cnt)),
            "allocated_equal": tuple(out2.shape) == (n, width)
            and bool(np.array_equal(out2.cpu().numpy().view(np.uint64), want))
            and bool(np.array_equal(st2.cpu().numpy(), st))
            and bool(np.array_equal(cnt2.cpu().numpy().view(np.uint64), cnt)),
            "refused": {
                "non_contiguous": refused(lambda: ctx.set_args_tensor("mix", T.MIX_P, wrong[:, :7])),
                "cpu": refused(lambda: ctx.set_args_tensor("mix", T.MIX_P, t.cpu())),
                "dtype": refused(lambda: ctx.set_args_tensor("mix", T.MIX_P, t.to(torch.float64))),
                "out_non_contiguous": refused(lambda: ctx.results_tensor(4, out=wrong[:, :7])),
                "out_cpu": refused(lambda: ctx.results_tensor(4, out=wrong.cpu())),
                "out_dtype": refused(lambda: ctx.results_tensor(4, out=wrong.to(torch.int32))),
            },
        }
    finally:
        ctx.close()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
