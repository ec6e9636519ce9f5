"""What mixed call vectors cost (WasmEdge_BatchSetCalls, DESIGN.md "Per-instance calls"):
one module with two exports of different character -- A, a recursive fib, and B, a branchy
br_table loop -- at 64K instances, the interpreter kernel's time for

  1. every instance calling A;
  2. every instance calling B;
  3. A and B interleaved lane by lane (every wave holds both);
  4. A and B in alternating whole waves (every wave holds one).

(3) and (4) do half of (1)'s and half of (2)'s work. A wave runs its functions one after
the other, so (3) is expected near (1) + (2) and (4) near half of that: the gap is what a
caller gains by grouping requests by wave. A probe, no pass mark: it prints what it finds.

Timing: the HIP-event time of the kernel alone (WasmEdge_BatchRun's KernelSeconds), after
two warm-up runs per vector (code objects, the longest-first wave order of that vector),
the median and the spread of --runs repeats; the four vectors are taken in turn, round by
round, so that drift of the machine falls on all of them alike. Results are checked against
the oracle on a sample of instances first.

  python tools/mixed_calls_probe.py [--instances 65536] [--runs 7] [--fib 23] [--iters 20000]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from wasmedge_amd import batch  # noqa: E402
from wasmedge_amd.wat import assemble  # noqa: E402

I32 = batch.I32

WAT = r"""
(module
  (func $fib (export "fib") (param $n i32) (result i32)
    (if (result i32) (i32.lt_u (local.get $n) (i32.const 2))
      (then (local.get $n))
      (else (i32.add (call $fib (i32.sub (local.get $n) (i32.const 1)))
                     (call $fib (i32.sub (local.get $n) (i32.const 2)))))))
  ;; a state machine over a per-instance xorshift stream: the state picks the arm
  (func (export "walk") (param $x i32) (param $iters i32) (result i32)
    (local $i i32) (local $acc i32)
    (local.set $x (i32.or (local.get $x) (i32.const 1)))
    (block $done
      (loop $l
        (br_if $done (i32.ge_u (local.get $i) (local.get $iters)))
        (local.set $i (i32.add (local.get $i) (i32.const 1)))
        (local.set $x (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 13))))
        (local.set $x (i32.xor (local.get $x) (i32.shr_u (local.get $x) (i32.const 17))))
        (local.set $x (i32.xor (local.get $x) (i32.shl (local.get $x) (i32.const 5))))
        (block $b3
          (block $b2
            (block $b1
              (block $b0
                (br_table $b0 $b1 $b2 $b3 (i32.and (local.get $x) (i32.const 3))))
              (local.set $acc (i32.add (local.get $acc) (local.get $x)))
              (br $l))
            (local.set $acc (i32.xor (local.get $acc) (i32.rotl (local.get $x) (i32.const 7))))
            (br $l))
          (local.set $acc (i32.sub (i32.mul (local.get $acc) (i32.const 3)) (local.get $i)))
          (br $l))
        (local.set $acc (i32.add (local.get $acc) (i32.popcnt (local.get $x))))
        (br $l)))
    (local.get $acc)))
"""


def vector(kind, n, fib_n, iters):
    """(func_of, rows) of the n instances for layout 1..4."""
    pick = {1: lambda i: 0, 2: lambda i: 1, 3: lambda i: i & 1, 4: lambda i: (i >> 6) & 1}[kind]
    func_of = [pick(i) for i in range(n)]
    rows = [[(fib_n, I32)] if f == 0 else [(i * 2654435761 & 0xFFFFFFFF, I32), (iters, I32)]
            for i, f in enumerate(func_of)]
    return func_of, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--fib", type=int, default=23)
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    wasm = assemble(WAT)
    n = args.instances
    names = ["fib", "walk"]
    labels = {1: "all A (fib)", 2: "all B (walk)", 3: "A/B by lane", 4: "A/B by wave"}
    ctxs, counts = {}, {}
    import oracle_py
    m = oracle_py.Module(wasm)
    for kind in (1, 2, 3, 4):
        # a context per vector: each keeps its own staged calls and learned wave order
        ctx = batch.BatchContext(wasm, n, device=args.device)
        func_of, rows = vector(kind, n, args.fib, args.iters)
        ctx.set_calls(names, func_of, rows)
        for _ in range(2):
            ctx.run()
        rets, st, cnt = ctx.results(1)
        ints = batch.ret_ints(rets)
        for i in range(0, n, max(1, n // 16)):
            code, ref, rcnt, _ = m.run(names[func_of[i]], [v for v, _ in rows[i]])
            assert (int(st[i]), int(ints[i][0]), int(cnt[i])) == (code, ref[0], rcnt), (kind, i)
        ctxs[kind], counts[kind] = ctx, int(cnt.sum())
    times = {k: [] for k in ctxs}
    for _ in range(args.runs):
        for kind, ctx in ctxs.items():
            times[kind].append(ctx.run())
    out = {"instances": n, "fib": args.fib, "iters": args.iters, "runs": args.runs,
           "engine": ctxs[1].engine(), "layouts": {}}
    for kind in ctxs:
        t = times[kind]
        out["layouts"][labels[kind]] = {"kernel_ms_median": 1e3 * statistics.median(t),
                                        "kernel_ms_min": 1e3 * min(t), "kernel_ms_max": 1e3 * max(t),
                                        "instructions": counts[kind]}
        print("%-14s kernel %8.3f ms median (%.3f .. %.3f), %.3e instructions"
              % (labels[kind], 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t), counts[kind]))
    med = {k: statistics.median(times[k]) for k in times}
    both = med[1] + med[2]
    print("(1) + (2) = %.3f ms; by lane %.2fx of it, by wave %.2fx of it"
          % (1e3 * both, med[3] / both, med[4] / both))
    print(json.dumps(out))
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
