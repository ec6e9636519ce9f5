"""Run by tests/test_memspans.py in a process of its own: the tensor variants of the
device-resident spans transfer. torch initialises its device BEFORE the first BatchContext
exists -- a torch build with a HIP runtime of its own finds no GPU when it starts second, and
the test suite's process has long created contexts. Prints one JSON line: per granule and
case, whether rows, status bytes and the out-of-bounds count equal the host variants' for the
same spans.

    python tests/memspans_tensor_child.py
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

from wasmedge_amd import batch          # noqa: E402
from wasmedge_amd.wat import assemble   # noqa: E402
import test_memio as T                  # noqa: E402
import test_memspans as S               # noqa: E402

N = T.N


def compare(ctx, offsets, lens, offset, length, width, tiled):
    """read and write through the tensor variants with `offsets` / `lens` (int64 device
    tensors or views, or None) against the host variants with the same spans"""
    h_off = offsets.cpu().numpy().astype(np.uint32) if offsets is not None else None
    h_len = lens.cpu().numpy().astype(np.uint32) if lens is not None else None
    # read
    host = np.full((N, width), 0x77, np.uint8)
    _, st_h = ctx.read_memories(length, offset=offset, offsets=h_off, lens=h_len, out=host)
    t = torch.full((N, width), 0x77, dtype=torch.uint8, device="cuda:0")
    st = torch.full((N,), 0x77, dtype=torch.uint8, device="cuda:0")
    oob = ctx.read_memories_spans_tensor(t, offsets=offsets, lens=lens, offset=offset, length=length, status=st)
    tiled_r = ctx.last_spans_tiled_waves()
    read_ok = bool(np.array_equal(t.cpu().numpy(), host))
    st_ok = bool(np.array_equal(st.cpu().numpy(), st_h))
    n_ok = oob == int((st_h != 0).sum())
    # write: what the host variant then reads at the same spans is the rows' bytes
    rows = np.random.default_rng(width).integers(1, 256, (N, width), dtype=np.uint8)
    st.fill_(0x77)
    oob = ctx.write_memories_spans_tensor(torch.from_numpy(rows).to("cuda:0"), offsets=offsets, lens=lens,
                                          offset=offset, length=length, status=st)
    tiled_w = ctx.last_spans_tiled_waves()
    back = np.full((N, width), 0x77, np.uint8)
    _, st_h2 = ctx.read_memories(length, offset=offset, offsets=h_off, lens=h_len, out=back)
    want = np.full((N, width), 0x77, np.uint8)
    for i in range(N):
        if st_h[i] == 0:
            k = int(h_len[i]) if h_len is not None else length
            want[i, :k] = rows[i, :k]
    return {"read_equals_host": read_ok,
            "write_equals_host": bool(np.array_equal(back, want)) and bool(np.array_equal(st_h2, st_h)),
            "status_equals_host": st_ok and bool(np.array_equal(st.cpu().numpy(), st_h)),
            "count_equals_host": bool(n_ok and oob == int((st_h != 0).sum())),
            "tiled_waves": [tiled_r, tiled_w], "tiled_expected": [tiled, tiled]}


def main():
    out = {}
    for granule in T.GRANULES:
        res = []
        # the columns of a results_tensor output, as views
        ctx = batch.BatchContext(assemble(S.OBS_WAT), N, device=0, memory_granule=granule)
        try:
            ctx.set_args("obs", batch.make_values([[i % 7] for i in range(N)], [T.I32]))
            ctx.run()
            slots, _, _ = ctx.results_tensor(2)
            res.append(compare(ctx, slots[:, 0], slots[:, 1], 0, 48, 52, 0))
        finally:
            ctx.close()
        # one start for everybody, near the end of the first page of instances of 1..3 pages
        os.environ["WB_RELAYOUT"] = "0"
        ctx = T.context(granule)
        try:
            T.run(ctx, "grow", [[i % 3] for i in range(N)], 1)
            T.run(ctx, "fill", [[i + 1, 65536 - 300, 300 + 4000 * (i % 3 > 0)] for i in range(N)], 0)
            offs = torch.full((N,), 65536 - 128, dtype=torch.int64, device="cuda:0")
            res.append(compare(ctx, offs, None, 0, 4096, 4096, 3))
        finally:
            ctx.close()
        out[str(granule)] = res
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
