"""Device-resident spans (WasmEdge_BatchWriteMemoriesSpansDevice / ReadMemoriesSpansDevice,
DESIGN.md "Device-resident spans") at 64K instances whose own offsets are all the same -- the
usual case, identical instances running the same allocator -- for granules 16 and 128 and
Len = 64, 4096 and 65536 bytes per instance:

  (a) "host_offsets": WriteMemoriesDevice / ReadMemoriesDevice with a host Offsets array, the
      only way before this call: the per-lane path, device allocations and copies per call;
  (b) "spans": the new calls with the same offsets in device slots and a status tensor
      ("spans_nostatus": PerInstance NULL);
  (c) "no_offsets": the Device variants without Offsets, the tiled ceiling.

Wall clock around the synchronous call, median of 7 after 2 warm-ups. Prints a table and
writes the numbers as JSON (default profiles/memspans_probe.json).

    python tools/memspans_probe.py [--instances 65536] [--out profiles/memspans_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from wasmedge_amd import batch          # noqa: E402
from wasmedge_amd.wat import assemble   # noqa: E402
from memio_probe import WAT, median_seconds   # noqa: E402

GRANULES = (16, 128)
LENS = (64, 4096, 65536)
OWN = 4096   # every instance's own offset


def main():
    import torch
    # (a torch with a HIP runtime of its own has to find its device before the library does)
    torch.zeros(1, device="cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memspans_probe.json"))
    args = ap.parse_args()
    n = args.instances
    wasm = assemble(WAT)
    host_offs = np.full(n, OWN, np.uint32)
    slots = torch.full((n,), OWN, dtype=torch.int64, device="cuda:0")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    rows = []
    for granule in GRANULES:
        ctx = batch.BatchContext(wasm, n, device=0, memory_granule=granule)
        try:
            for length in LENS:
                t = torch.randint(0, 256, (n, length), dtype=torch.uint8, device="cuda:0")
                u = torch.empty_like(t)
                ways = {
                    "host_offsets": (lambda: ctx.write_memories_tensor(t, offsets=host_offs),
                                     lambda: ctx.read_memories_tensor(u, offsets=host_offs)),
                    "spans": (lambda: ctx.write_memories_spans_tensor(t, offsets=slots, status=status),
                              lambda: ctx.read_memories_spans_tensor(u, offsets=slots, status=status)),
                    "spans_nostatus": (lambda: ctx.write_memories_spans_tensor(t, offsets=slots),
                                       lambda: ctx.read_memories_spans_tensor(u, offsets=slots)),
                    "no_offsets": (lambda: ctx.write_memories_tensor(t, offset=OWN),
                                   lambda: ctx.read_memories_tensor(u, offset=OWN)),
                }
                row = {"granule": granule, "len": length, "bytes": n * length}
                for name, (wr, rd) in ways.items():
                    ctx.reset()
                    u.zero_()
                    row[name] = {"write_s": median_seconds(wr), "read_s": median_seconds(rd)}
                    assert torch.equal(t, u), name
                    if name.startswith("spans"):
                        row["tiled_waves"] = ctx.last_spans_tiled_waves()
                rows.append(row)
                del t, u
        finally:
            ctx.close()
    for r in rows:
        print("granule %3d len %5d  " % (r["granule"], r["len"]) + "  ".join(
            "%s w %.1f r %.1f us" % (k, r[k]["write_s"] * 1e6, r[k]["read_s"] * 1e6)
            for k in ("host_offsets", "spans", "spans_nostatus", "no_offsets")) + "  tiled waves %d" % r["tiled_waves"])
    with open(args.out, "w") as f:
        json.dump({"instances": n, "own_offset": OWN, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
