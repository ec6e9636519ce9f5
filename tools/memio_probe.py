"""Bulk memory transfer rates (WasmEdge_BatchWriteMemories / ReadMemories, DESIGN.md "Bulk
memory transfer") at 64K instances, for each interleave granule:

  * the device variants for Len = 64, 4096 and 65536 bytes per instance, beside a torch
    device-to-device copy of the same byte count taken in the same process (the yardstick);
  * the host variants for Len = 64 and 4096.

Wall clock around the synchronous call, median of 7 after 2 warm-ups. Prints a table and
writes the numbers as JSON (default profiles/memio_probe.json).

    python tools/memio_probe.py [--instances 65536] [--out profiles/memio_probe.json]
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

WAT = '(module (memory (export "memory") 2 2) (func (export "nop")))'
GRANULES = (4, 8, 16, 128)
DEVICE_LENS = (64, 4096, 65536)
HOST_LENS = (64, 4096)


def median_seconds(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    import torch
    # (a torch with a HIP runtime of its own has to find its device before the library does)
    torch.zeros(1, device="cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memio_probe.json"))
    args = ap.parse_args()
    n = args.instances
    wasm = assemble(WAT)
    rows = []
    for granule in GRANULES:
        ctx = batch.BatchContext(wasm, n, device=0, memory_granule=granule)
        try:
            for length in DEVICE_LENS:
                t = torch.randint(0, 256, (n, length), dtype=torch.uint8, device="cuda:0")
                u = torch.empty_like(t)

                def copy():
                    u.copy_(t)
                    torch.cuda.synchronize()
                nbytes = n * length
                ref = median_seconds(copy)
                wr = median_seconds(lambda: ctx.write_memories_tensor(t, offset=4096))
                rd = median_seconds(lambda: ctx.read_memories_tensor(u, offset=4096))
                assert torch.equal(t, u)
                rows.append({"granule": granule, "len": length, "where": "device", "bytes": nbytes,
                             "copy_Bps": nbytes / ref, "write_Bps": nbytes / wr, "read_Bps": nbytes / rd,
                             "write_frac": ref / wr, "read_frac": ref / rd})
                del t, u
            for length in HOST_LENS:
                a = np.random.default_rng(length).integers(0, 256, (n, length), dtype=np.uint8)
                nbytes = n * length
                wr = median_seconds(lambda: ctx.write_memories(a, offset=4096))
                rd = median_seconds(lambda: ctx.read_memories(length, offset=4096))
                assert np.array_equal(ctx.read_memories(length, offset=4096)[0], a)
                rows.append({"granule": granule, "len": length, "where": "host", "bytes": nbytes,
                             "write_Bps": nbytes / wr, "read_Bps": nbytes / rd})
        finally:
            ctx.close()
    for r in rows:
        line = "granule %3d  %-6s len %5d  write %8.2f GB/s  read %8.2f GB/s" % (
            r["granule"], r["where"], r["len"], r["write_Bps"] / 1e9, r["read_Bps"] / 1e9)
        if r["where"] == "device":
            line += "  copy %8.2f GB/s  write %.2f  read %.2f of it" % (
                r["copy_Bps"] / 1e9, r["write_frac"], r["read_frac"])
        print(line)
    with open(args.out, "w") as f:
        json.dump({"instances": n, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
