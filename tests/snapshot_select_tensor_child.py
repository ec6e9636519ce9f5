"""Run by tests/test_snapshot_select.py in a process of its own: restore_tensor, the torch
mirror of WasmEdge_BatchSnapshotRestoreSelectedDevice. torch initialises its device BEFORE the
first BatchContext exists -- a torch build with a HIP runtime of its own finds no GPU when it
starts second, and the test suite's process has long created contexts. The map is built on the
device: the statuses of a run go into a tensor, and torch.where keeps the instances that
returned and restores the ones that trapped. Prints one JSON line: whether the tensor path
equals restore_selected with the same map on the count, the memory hashes and sum().

    python tests/snapshot_select_tensor_child.py
"""
import json
import os
import sys

import torch

torch.cuda.init()
torch.zeros(1, device="cuda:0")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_snapshot as T     # noqa: E402


def main():
    n = T.N
    ctx = T.context(4)
    try:
        T.gpu_call(ctx, "init", T.SEEDS, 0)
        snap = ctx.snapshot()
        seen = []
        for tensor in (False, True):
            if seen:
                ctx.restore(snap)
            T.gpu_call(ctx, "step", T.XS, 1)
            _, status, _ = ctx.results_tensor(1)
            ident = torch.arange(n, dtype=torch.int32, device=status.device)
            src = torch.where(status != 0, ident, torch.full_like(ident, -1))   # trapped: start over
            kept = int((src == -1).sum())
            if tensor:
                _, restored = ctx.restore_tensor(snap, src)
            else:
                _, restored = ctx.restore_selected(snap, [int(x) for x in src.cpu()])
            gone = False
            try:
                ctx.results(1)
            except Exception:
                gone = True
            hashes = [int(h) for h in ctx.memory_hash()]
            rets, st, cnt = T.gpu_call(ctx, "sum", T.NONE, 1)
            seen.append((kept, restored, gone, hashes, rets, [int(x) for x in st], [int(x) for x in cnt]))
        a, b = seen
        res = {"kept": b[0], "restored": b[1], "restored_equal": a[1] == b[1] and a[0] == b[0],
               "results_gone": a[2] and b[2], "hashes_equal": a[3] == b[3], "sums_equal": a[4:] == b[4:]}
        snap.close()
    finally:
        ctx.close()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
