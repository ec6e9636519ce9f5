"""A static issue model of a compiled loop's VALU code (test helper; DESIGN.md "Results
(chain-loop tail)").

One wave per SIMD issues an instruction every 4 cycles; an instruction that reads a
register waits until `lat(producer, consumer)` cycles after the producer's issue. The
block runs twice back to back, so the second trip sees the loop-carried producers; the
stall cycles of that second trip are the result. LATENCY is the table measured with
tools/ubench/valu_lat.hip on an MI355X (profiles/chaintail_valu_lat.txt): every class and
every producer -> consumer pair of the chain loop reads 4.0 cycles per instruction along a
dependent chain, which is the issue interval itself."""
import re

ISSUE = 4
LATENCY = {"v_xor_b32": 4, "v_add_u32": 4, "v_add3_u32": 4, "v_alignbit_b32": 4}
DEFAULT = 4


def _regs(tok):
    out = []
    for m in re.finditer(r"\b([vs])(?:(\d+)|\[(\d+):(\d+)\])", tok):
        base = 0 if m.group(1) == "v" else 1000
        if m.group(2) is not None:
            out.append(base + int(m.group(2)))
        else:
            out += [base + r for r in range(int(m.group(3)), int(m.group(4)) + 1)]
    if re.search(r"\bvcc\b", tok):
        out.append(2000)
    return out


def parse(lines):
    """(class, defs, uses) of every v_ line"""
    ins = []
    for ln in lines:
        if not ln.startswith("v_"):
            continue
        mn, _, rest = ln.partition(" ")
        ops = rest.split(", ")
        cls = re.sub(r"_e(32|64)$", "", mn)
        ins.append((cls, _regs(ops[0]), [r for o in ops[1:] for r in _regs(o)]))
    return ins


def stall_cycles(lines, lat=None):
    """stall cycles of the second of two back-to-back trips through `lines`"""
    ins = parse(lines)
    lat = lat or (lambda prod, cons: LATENCY.get(prod, DEFAULT))
    ready = {}   # register -> (cycle its value is usable, producer class)
    clock, stalls = 0, 0
    for trip in range(2):
        for cls, defs, uses in ins:
            t = clock
            for r in uses:
                if r in ready:
                    issued, prod = ready[r]
                    t = max(t, issued + lat(prod, cls))
            if trip:
                stalls += t - clock
            for r in defs:
                ready[r] = (t, cls)
            clock = t + ISSUE
    return stalls
