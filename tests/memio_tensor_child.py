"""Run by tests/test_memio.py in a process of its own: the tensor variants of the bulk
transfer. torch initialises its device BEFORE the first BatchContext exists -- a torch build
with a HIP runtime of its own finds no GPU when it starts second, and the test suite's
process has long created contexts. Prints one JSON line: per granule and case, whether the
tensor results equal the host variants' and numpy's expectation.

    python tests/memio_tensor_child.py
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
import test_memio as T           # noqa: E402


def main():
    out = {}
    for granule in T.GRANULES:
        rng = np.random.default_rng(400 + granule)
        ctx = T.context(granule)
        res = []
        try:
            # 16-byte rows, 4-byte rows, per-instance offsets and lengths
            for width, offset, per_instance in ((4096, 256, False), (68, 260, False), (67, 3, True)):
                offs = np.array([(i * 37) % 509 for i in range(T.N)], np.uint32) if per_instance else None
                lens = np.array([i % (width + 1) for i in range(T.N)], np.uint32) if per_instance else None
                rows = rng.integers(0, 256, (T.N, width), dtype=np.uint8)
                ctx.reset()
                st_w = ctx.write_memories_tensor(torch.from_numpy(rows).to("cuda:0"), offset=offset,
                                                 offsets=offs, lens=lens)
                host, st_h = ctx.read_memories(width, offset=offset, offsets=offs, lens=lens)
                want = np.zeros((T.N, width), np.uint8)
                for i in range(T.N):
                    k = int(lens[i]) if per_instance else width
                    want[i, :k] = rows[i, :k]
                t = torch.zeros((T.N, width), dtype=torch.uint8, device="cuda:0")
                st_r = ctx.read_memories_tensor(t, offset=offset, offsets=offs, lens=lens)
                got = [int(x) for x in T.run(ctx, "sum", [[offset, width]] * T.N, 1)] if not per_instance else None
                res.append({"case": [width, offset, per_instance],
                            "status_clear": not (st_w.any() or st_h.any() or st_r.any()),
                            "host_equals_numpy": bool(np.array_equal(host, want)),
                            "tensor_equals_host": bool(np.array_equal(t.cpu().numpy(), host)),
                            "sum_equals_numpy": got is None or got == [int(x) for x in T.np_sum(rows)]})
        finally:
            ctx.close()
        out[str(granule)] = res
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
