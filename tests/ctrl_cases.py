"""Seeded random modules of structured control flow for the parity tests
(tests/test_ctrl_random.py; DESIGN.md "Parity tests").

The other generators (tests/test_jit.py, tests/float_cases.py) emit one statement shape,
(local.set $d (op operands)), inside a fixed skeleton: nothing lives on the operand stack
across a label, no block has parameters or results, no branch carries or unwinds a value,
no code follows an unconditional branch. This one goes where the frontend's lowering is
intricate (frontend.cpp: lazy K_LOCAL / K_CONST entries and materialize_locals,
move_top_to / top_in_place, try_retarget, the per-branch count corrections, pop_any in dead
code) and where the SIMT scheduler parks lanes at many pcs. Value semantics are not the
point: the ops are cheap integer ones, and one f64 and one v128 local make values of 2 and
4 cells cross labels.

ctrl_module(seed, tail=False, runs=True) -> wasm bytes; ctrl_wat(...) -> the text (bodies
in the flat form). tail=True adds return_call from inside nested blocks (the TailCall
proposal). runs=False is the count-only twin: the same module without the generated
nop / drop / select runs, which must return the same values.

Functions: run(s) -> i64 (exported), the helpers $h0 < $h1 < $h2 and the recursive $rec, all
of the type (i32, i64) -> i64, and $w of another type for the table. Every function has the
locals $s (the per-lane seed, never written), $a $b $t (i32), $p $q (i64), $f (f64), $v
(v128) and $fuel.

Termination, by construction:
  * every loop back edge is the loop's own last br_if, and-ed with `--$fuel > 0`; $fuel is
    set once per function entry (FUEL) and only these edges write it
  * no other generated branch targets a loop label (dead code included)
  * a function calls only functions of a lower rank (RANK: run > $h2 > $h1 > $rec > $h0); the
    table holds helpers only and only run calls through it
  * $rec calls itself with $p - 1 behind `$p != 0`, after clamping $p to at most 12 on entry

Memory (one page): ARMS + 16 j + min(index, 15) gets a 1 before the j-th br_table runs
(which arms the rows took), random stores into SCRATCH..SCRATCH+4K, run's locals at FINAL."""
import random

from wasmedge_amd.wat import assemble

ARMS, SCRATCH, FINAL = 0x400, 0x1000, 0x8000
FUEL = {"run": 10, "h2": 4, "h1": 4, "h0": 3, "rec": 2}
RANK = {"run": 4, "h2": 3, "h1": 2, "rec": 1, "h0": 0}
MAXD = 5
TABLE = ["$h0", "$h1", "$h2", "$w"]       # entries 4 and 5 are null; the table has 6
BAD_INDEX = {"type": 3, "null": 4, "range": 9}
LONG_RUNS = [("label", 255), ("label", 256), ("loop", 255), ("loop", 256), ("branch", 255),
             ("branch", 256), ("retarget", 127), ("retarget", 128)]      # by seed % 8: every module has one
LONGER_RUNS = {0: ("branch", 300), 2: ("label", 300), 5: ("loop", 300)}  # by seed % 8

# the constructs that must occur over a committed seed set (cov tags, see constructs())
REQUIRED = sorted(
    [(k, "res", n) for k in ("block", "loop", "if") for n in (0, 1, 2)] +
    [(k, "par", n) for k in ("block", "loop", "if") for n in (1, 2)] +
    [("if_noelse", "par", n) for n in (1, 2)] +
    [(op, "arity", n) for op in ("br", "br_if", "br_table") for n in (0, 1, 2)] +
    [(op, "depth", n) for op in ("br", "br_if", "br_table") for n in (0, 1, 2, 3)] +
    [(op, "junk", 1) for op in ("br", "br_if", "br_table")] +
    [(op, "cells", n) for op in ("br", "br_if", "br_table") for n in (2, 4)] +
    [("br_if", "fallthrough", 1), ("br_table", "repeat", 1), ("br_table", "mixed", 1),
     ("loop", "reenter", 1), ("loop", "reenter", 2), ("loop", "exit2", 1),
     ("return", "depth3", 1), ("return", "loop_callee", 1)] +
    [("dead_after", k, 1) for k in ("br", "br_table", "return", "unreachable")] +
    [("dead", k, 1) for k in ("pops", "set", "block", "br_if")] +
    [("label", "dead_only", 1), ("label", "unreached", 1)] +
    [("stale", k, 1) for k in ("set", "tee", "set_wide", "tee_wide")] +
    [("retarget", k, 1) for k in ("label", "nops", "const_label", "const_nops")] +
    [("run", pos, n) for pos, n in LONG_RUNS + list(LONGER_RUNS.values())] +
    [("run", pos, 1) for pos in ("label", "loop", "branch")] +
    [("runkind", k, 1) for k in ("nop", "drop", "select", "local")] +
    [("call", k, 1) for k in ("divergent", "indirect", "recursion")] +
    [("indirect_trap", k, 1) for k in BAD_INDEX] +
    [("trap", k, 1) for k in ("unreachable", "div", "oob")], key=str)
REQUIRED_TAIL = [("return_call", "nested", 1)]
TRAP_CODES = {0x84, 0x88, 0x89, 0x8A, 0x8B, 0x8C}   # div, oob, unreachable, null, range, type


class _Gen:
    def __init__(self, seed, tail=False, runs=True):
        self.r = random.Random("ctrl/%d/%d" % (seed, tail))
        self.seed, self.tail, self.runs = seed, tail, runs
        self.cov = set()
        self.decks = {}
        self.tables = []          # per br_table: its number of entries before the default
        self.labels = []
        self.fn = "run"
        self.budget = 0
        self.bad_done = False
        self.want_return = False

    def tag(self, a, b, c=1):
        self.cov.add((a, b, c))

    def pick(self, key, items):
        """the next item of a deck: `items` in an order fixed per key, walked cyclically from
        a start that depends on the seed, so that seeds 0..7 cover a deck together"""
        if key not in self.decks:
            order = list(items)
            random.Random("ctrl/" + key).shuffle(order)
            self.decks[key] = [order, (self.seed % 8) * len(order) // 8]
        d = self.decks[key]
        d[1] += 1
        return d[0][(d[1] - 1) % len(d[0])]

    # ---- values
    def ty(self):
        return self.pick("ty", ["i32", "i64", "i32", "f64", "i64", "v128", "i32"])

    def local(self, t, write=False):
        if t == "i32":
            return self.r.choice(["$a", "$b"])
        if t == "i64":
            return "$q" if write and self.fn == "rec" else self.r.choice(["$p", "$q"])
        return "$f" if t == "f64" else "$v"

    def lane(self, mask, plus=None):
        """some bits of the read-only seed, scrambled: ((s [+ local]) * odd) >> 20, masked"""
        odd = self.r.randrange(1 << 31) * 2 + 1
        src = ["local.get $s"] + (["local.get " + plus, "i32.add"] if plus else [])
        return src + ["i32.const %d" % odd, "i32.mul", "i32.const 20", "i32.shr_u", "i32.const %d" % mask, "i32.and"]

    def cond(self, one_in):
        """an i32 that is nonzero on about one lane in `one_in` (a power of two)"""
        k = self.r.randrange(4)
        if k == 0:
            return self.lane(one_in - 1) + ["i32.eqz"]
        if k == 1:
            return self.lane(one_in - 1) + ["i32.const %d" % self.r.randrange(one_in), "i32.eq"]
        if k == 2:
            return self.lane(2 * one_in - 1) + ["i32.const 2", "i32.lt_u"]
        return self.lane(one_in - 1) + ["i32.const 1", "i32.lt_s"]

    def val(self, t):
        r = self.r
        k = r.randrange(5)
        x = self.local(t)
        if t == "i32":
            return [["local.get " + x], ["i32.const %d" % r.randrange(-9, 1000)],
                    ["local.get " + x, "i32.const %d" % r.randrange(1, 99), "i32.add"],
                    self.lane(0xFFFF), ["local.get $a", "local.get $b", "i32.xor"]][k]
        if t == "i64":
            return [["local.get " + x], ["i64.const %d" % r.randrange(-9, 1 << 40)],
                    ["local.get " + x, "i64.const %d" % r.randrange(1, 99), "i64.add"],
                    ["local.get $a", "i64.extend_i32_u"], ["local.get $p", "local.get $q", "i64.xor"]][k]
        if t == "f64":
            return [["local.get $f"], ["f64.const %s" % r.choice(["0", "-0", "1.5", "-3", "1e10"])],
                    ["local.get $a", "f64.convert_i32_s"], ["local.get $f", "f64.neg"], ["local.get $f"]][k]
        return [["local.get $v"], ["v128.const i32x4 1 -2 3 0x7fffffff"], ["local.get $a", "i32x4.splat"],
                ["local.get $p", "i64x2.splat"], ["local.get $v", "local.get $b", "i32x4.splat", "i32x4.add"]][k]

    def vals(self, ts):
        return [x for t in ts for x in self.val(t)]

    def sink(self, t):
        r = self.r
        k = r.randrange(3)
        x = self.local(t, write=True)
        if t == "i32":
            return [["local.set " + x], ["local.get " + x, "i32.add", "local.set " + x],
                    ["local.get " + x, "i32.const 5", "i32.rotl", "i32.xor", "local.set " + x]][k]
        if t == "i64":
            return [["local.set " + x], ["local.get " + x, "i64.xor", "local.set " + x],
                    ["local.get $q", "i64.const 9", "i64.rotl", "i64.add", "local.set $q"]][k]
        if t == "f64":
            return [["local.set $f"], ["i64.reinterpret_f64", "local.get $q", "i64.xor", "local.set $q"],
                    ["f64.abs", "local.set $f"]][k]
        return [["local.set $v"], ["local.get $v", "v128.xor", "local.set $v"],
                ["i64x2.extract_lane %d" % r.randrange(2), "local.get $q", "i64.add", "local.set $q"]][k]

    def sinks(self, ts):
        return [x for t in reversed(ts) for x in self.sink(t)]

    def tweak(self, t):
        """change the top of the stack in place"""
        return {"i32": ["i32.const 1", "i32.add"], "i64": ["i64.const 3", "i64.mul"], "f64": ["f64.neg"],
                "v128": ["local.get $v", "v128.xor"]}[t]

    def junk(self, lo=0):
        ts = [self.ty() for _ in range(self.pick("junk", [1, 0, 2, 1, 1, 3]))]
        if not ts and lo:
            ts = [self.ty()]
        return self.vals(ts), ts

    def sarg(self):
        return self.r.choice([["local.get $s", "i32.const %d" % self.r.randrange(1, 1 << 20), "i32.add"],
                              ["local.get $s", "local.get $a", "i32.xor"]])

    @staticmethod
    def bt(P, R):
        return ((" (param %s)" % " ".join(P)) if P else "") + ((" (result %s)" % " ".join(R)) if R else "")

    def push(self, kind, types):
        self.labels.append((kind, list(types)))

    def cells(self, op, ts):
        for t in ts:
            if t in ("i64", "f64"):
                self.tag(op, "cells", 2)
            if t == "v128":
                self.tag(op, "cells", 4)

    def branch_tags(self, op, depth, jt):
        ts = self.labels[len(self.labels) - 1 - depth][1]
        assert self.labels[len(self.labels) - 1 - depth][0] != "loop"
        self.tag(op, "arity", len(ts))
        self.tag(op, "depth", min(depth, 3))
        if jt:
            self.tag(op, "junk")
            self.cells(op, ts)

    # ---- runs of folded instructions (nothing of them reaches the device but their count)
    def run(self, pos, n=None):
        r = self.r
        if n is None:
            n = self.pick("runlen", [1, 2, 3, 1, 5, 2, 17, 4, 1, 40, 3, 2])
        kind = self.pick("runkind", ["nop", "drop", "nop", "select", "local", "nop", "drop"])
        if n >= 100:
            kind = self.pick("runkind_long", ["nop", "nop", "drop", "nop"])
        x = r.choice(["$a", "$b"])
        unit = {"nop": ["nop"], "drop": ["i32.const %d" % r.randrange(9), "drop"], "local": ["local.get " + x, "drop"],
                "select": ["i32.const 1", "i32.const 2", "i32.const %d" % r.randrange(2), "select", "drop"]}[kind]
        out = unit * (n // len(unit)) + ["nop"] * (n % len(unit))
        self.tag("run", pos, n if n >= 100 else 1)
        self.tag("runkind", kind)
        return out if self.runs else []

    # ---- dead code, directly before the `end` of a block or if (never of a loop)
    def dead(self, after):
        assert self.labels[-1][0] != "loop"
        self.tag("dead_after", after)
        out = []
        kinds = {self.pick("dead", ["pops", "set", "block", "br_if", "pops", "block"]) for _ in range(self.r.randrange(1, 3))}
        for k in ("pops", "set", "block", "br_if"):    # (br_if 0 last: it leaves the label's types)
            if k not in kinds:
                continue
            self.tag("dead", k)
            out += {"pops": ["drop", "drop", "i32.add", "local.set $a"],
                    "set": ["local.set $b", "i64.const 1", "local.set $q"],
                    "block": ["block", "i32.const 1", "br_if 0", "local.get $a", "local.set $b", "br 0", "end"],
                    "br_if": ["br_if 0"]}[k]
        return out

    # ---- statements (each leaves the stack as it found it)
    def simple(self):
        t = self.ty()
        return self.val(t) + self.sink(t)

    def store(self):
        t = self.ty()
        n = {"i32": 4, "i64": 8, "f64": 8, "v128": 16}[t]
        return self.lane(0xFFF & ~(n - 1)) + self.val(t) + ["%s.store offset=%d" % (t, SCRATCH + self.r.choice([0, 16, 256]))]

    def inner(self, depth, n=None):
        out = []
        for _ in range(self.r.randrange(1, 3) if n is None else n):
            out += self.stmt(depth)
        return out

    def body(self, kind, P, R, depth):
        """the body of a block / loop / if arm: P on the stack at its start, R at its end"""
        r = self.r
        out = []
        if P == R and P and (kind == "if" or r.random() < 0.5):
            out += self.tweak(P[-1])
            return out + self.inner(depth, 1)          # (P sits on the stack across its labels)
        out += self.sinks(P) + self.inner(depth)
        if kind != "loop" and r.random() < 0.3:        # leave by a br 0 over junk; dead code follows
            j, jt = self.junk(1)
            self.branch_tags("br", 0, jt)
            return out + j + self.vals(R) + ["br 0"] + self.dead("br")
        for t in R:
            out += self.val(t)
            if r.random() < 0.4:
                out += self.inner(depth, 1)
        return out

    def k_block(self, depth):
        kind = self.pick("bk", ["block", "loop", "if", "ifelse", "block", "ifelse", "loop", "if"])
        P = [self.ty() for _ in range(self.pick("bp" + kind, [0, 1, 2, 0, 1, 2, 0]))]
        R = [self.ty() for _ in range(self.pick("br" + kind, [0, 1, 2, 1, 0, 2]))]
        if kind == "if":       # without else: the parameters are the results
            R = list(P)
            if P:
                self.tag("if_noelse", "par", len(P))
        name = "if" if kind == "ifelse" else kind
        self.tag(name, "res", len(R))
        if P:
            self.tag(name, "par", len(P))
        out = self.vals(P)
        if name == "if":
            out += self.cond(2)
        out.append(name + self.bt(P, R))
        self.push(name, P if kind == "loop" else R)
        out += self.body(kind, P, R, depth + 1)
        if kind == "ifelse":
            out.append("else")
            out += self.body(kind, P, R, depth + 1)
        self.labels.pop()
        return out + ["end"] + self.sinks(R)

    def back_edge(self):
        return ["local.get $fuel", "i32.const 1", "i32.sub", "local.tee $fuel", "i32.const 0", "i32.gt_s"] + \
            self.lane(3, "$fuel") + ["i32.const 0", "i32.ne", "i32.and", "br_if 0"]

    def exit2(self):
        """leave the enclosing loop from two blocks inside it, to a label outside it"""
        loop_at = max(k for k, l in enumerate(self.labels) if l[0] == "loop")
        at = self.r.choice([k for k in range(loop_at) if self.labels[k][0] != "loop"])
        out = []
        j1, t1 = self.junk()
        out += j1 + ["block"]
        self.push("block", [])
        j2, t2 = self.junk()
        out += j2 + ["block"]
        self.push("block", [])
        depth = len(self.labels) - 1 - at
        ts = self.labels[at][1]
        self.branch_tags("br_if", depth, t1 + t2)
        self.tag("loop", "exit2")
        out += self.vals(ts) + self.cond(8) + ["br_if %d" % depth] + self.sinks(ts)
        self.labels.pop()
        out += ["end"] + ["drop"] * len(t2)
        self.labels.pop()
        return out + ["end"] + ["drop"] * len(t1)

    def k_loop(self, depth, long_run=None):
        P = [] if long_run else [self.ty() for _ in range(self.pick("lp", [0, 1, 2, 1, 2]))]
        keep = bool(P) and self.pick("lk", [False, True, True])
        R = P if keep else []
        out = self.store() if long_run else []
        out += self.vals(P)
        if long_run or self.r.random() < 0.4:
            out += self.run("loop", long_run)       # directly before the loop head
        out.append("loop" + self.bt(P, R))
        self.push("loop", P)
        self.tag("loop", "res", len(R))
        if P:
            self.tag("loop", "par", len(P))
            self.tag("loop", "reenter", len(P))
        out += self.sinks(P) + self.inner(depth + 1)
        if self.want_return:
            self.want_return = False
            out += self.k_return(depth + 1)
        if self.r.random() < 0.6:
            out += self.exit2()
        out += self.vals(P) + self.back_edge()
        if not keep:
            out += self.sinks(P)
        self.labels.pop()
        return out + ["end"] + self.sinks(R)

    def k_loopret(self, depth):
        self.want_return = True
        return self.k_loop(depth)

    def unwind(self, R, jt):
        """[jt R] on the stack -> [R]: a br 0 that carries R over the junk, or by hand"""
        if not jt:
            return []
        if self.labels[-1][0] != "loop" and self.labels[-1][1] == R and self.r.random() < 0.5:
            self.branch_tags("br", 0, jt)
            return ["br 0"] + self.dead("br")
        return self.sinks(R) + ["drop"] * len(jt) + self.vals(R)

    def nest(self, R, d, leaf):
        """d + 1 nested blocks of result R with junk between them; leaf() runs innermost"""
        out = ["block" + self.bt([], R)]
        self.push("block", R)
        self.tag("block", "res", len(R))
        if d == 0:
            out += leaf()
        else:
            j, jt = self.junk()
            out += j + self.nest(R, d - 1, leaf)
            if R and self.r.random() < 0.5:
                out += self.tweak(R[-1])
            if self.r.random() < 0.3:
                out += self.simple()
            out += self.unwind(R, jt)
        self.labels.pop()
        return out + ["end"]

    def k_nest(self, depth):
        op, arity, d = self.pick("nest", [(o, a, k) for o in ("br", "br_if", "br_table") for a in range(3) for k in range(4)])
        R = [self.pick("nty" + op, ["i32", "v128", "i64", "f64", "i32", "v128", "i64"]) for _ in range(arity)]
        r = self.r

        def br_if():
            j, jt = self.junk(1)
            self.branch_tags("br_if", d, jt)
            self.tag("br_if", "fallthrough")
            mid = self.run("branch") if d == 0 and r.random() < 0.5 else []
            return j + self.vals(R) + self.cond(2) + ["br_if %d" % d] + mid + self.unwind(R, jt)

        def br_arm():      # on some lanes, from inside an if
            out = self.cond(2) + ["if"]
            self.push("if", [])
            j, jt = self.junk(1)
            self.branch_tags("br", d, jt)
            out += j + self.vals(R) + ["br %d" % d] + self.dead("br")
            self.labels.pop()
            return out + ["end"] + self.vals(R)

        def br():
            j, jt = self.junk(1)
            self.branch_tags("br", d, jt)
            return j + self.vals(R) + ["br %d" % d] + self.dead("br")

        def br_table():
            n = r.randrange(2, 6)
            targets = [r.randrange(d + 1) for _ in range(n)] + [d]
            targets[r.randrange(n)] = d
            r.shuffle(targets)
            at = ARMS + 16 * len(self.tables)
            self.tables.append(n)
            j, jt = self.junk(1)
            for k in set(targets):
                self.branch_tags("br_table", k, jt)
            if len(set(targets)) < len(targets):
                self.tag("br_table", "repeat")
            if len(set(targets)) > 1:
                self.tag("br_table", "mixed")
            return self.lane(7) + ["local.tee $t", "i32.const 1", "i32.store8 offset=%d" % at] + j + self.vals(R) + \
                ["local.get $t", "br_table " + " ".join(map(str, targets))] + self.dead("br_table")

        if op == "br" and d > 0:
            out = self.nest(R, d - 1, br_arm)
        else:
            out = self.nest(R, d, {"br": br, "br_if": br_if, "br_table": br_table}[op])
        return out + self.sinks(R)

    def k_return(self, depth):
        out, drops = [], []
        for _ in range(self.r.randrange(2, 4)):
            j, jt = self.junk()
            out += j + ["block"]
            drops.append(len(jt))
            self.push("block", [])
        out += self.cond(16) + ["if"]
        self.push("if", [])
        j, jt = self.junk(1)
        out += self.store() + j
        lower = [f for f in ("h0", "h1", "h2") if RANK[f] < RANK[self.fn]]
        if self.tail and lower and self.fn != "run" and self.r.random() < 0.7:
            self.tag("return_call", "nested")
            out += self.sarg() + self.val("i64") + ["return_call $" + self.r.choice(lower)]
        else:
            self.tag("return", "depth3")
            if self.fn != "run" and any(l[0] == "loop" for l in self.labels):
                self.tag("return", "loop_callee")
            out += self.val("i64") + ["return"]
        out += self.dead("return")
        self.labels.pop()
        out.append("end")
        for n in reversed(drops):
            self.labels.pop()
            out += ["end"] + ["drop"] * n
        return out

    def k_trap(self, depth):
        kind = self.pick("trap", ["unreachable", "div", "oob"])
        self.tag("trap", kind)
        out = ["block", "block"] + self.cond(64) + ["if"]
        self.push("block", [])
        self.push("block", [])
        self.push("if", [])
        out += self.store() + ["i32.const %d" % self.r.randrange(100), "local.set $a"]
        if kind == "unreachable":
            out += ["unreachable"] + self.dead("unreachable")
        elif kind == "div":
            zero = ["local.get $s", "i32.const 0", "i32.and"]
            out += self.r.choice([["local.get $b"] + zero + ["i32.div_u", "local.set $b"],
                                  ["local.get $q"] + zero + ["i64.extend_i32_u", "i64.rem_s", "local.set $q"],
                                  ["local.get $b", "i32.const 0", "i32.rem_u", "local.set $b"]])
        else:
            out += self.r.choice([["i32.const 65533", "i32.load", "local.set $a"],
                                  ["local.get $a", "i32.const 65535", "i32.or", "i64.load offset=1", "local.set $q"],
                                  ["i32.const -4", "local.get $v", "v128.store offset=8"]])
        for _ in range(3):
            self.labels.pop()
        return out + ["end", "end", "end"]

    def k_call(self, depth, f=None):
        """a direct call to a lower rank inside a divergent arm, arguments over junk"""
        lower = [f for f in ("h0", "h1", "h2", "rec") if RANK[f] < RANK[self.fn]]
        if not lower:
            return self.simple()
        f = f or self.pick("callee" + self.fn, lower)
        self.tag("call", "divergent")
        j, jt = self.junk()
        if f == "rec":
            self.tag("call", "recursion")
            args = self.sarg() + self.lane(7) + ["i64.extend_i32_u"]
        else:
            args = self.sarg() + self.val("i64")
        return self.cond(2) + ["if"] + j + args + ["call $" + f] + self.sink("i64") + ["drop"] * len(jt) + ["end"]

    def k_indirect(self, depth):
        """call_indirect with a lane-divergent index over the three helpers (run only)"""
        self.tag("call", "indirect")
        j, jt = self.junk()
        out = j + self.sarg() + self.val("i64") + self.lane(3) + ["i32.const 3", "i32.rem_u",
                                                                   "call_indirect (type $h)"] + \
            self.sink("i64") + ["drop"] * len(jt)
        if not self.bad_done:      # once per module: an index that traps, on few lanes
            self.bad_done = True
            kind = self.pick("bad", ["type", "null", "range"])
            self.tag("indirect_trap", kind)
            out += ["block"] + self.cond(32) + ["if"] + self.store() + self.sarg() + self.val("i64") + \
                ["i32.const %d" % BAD_INDEX[kind], "call_indirect (type $h)", "local.set $q", "end", "end"]
        return out

    def k_stale(self, depth):
        """local.get $x left on the stack, $x overwritten deeper in the expression, both used"""
        t = self.ty()
        x = self.local(t, write=True)
        wide = "" if t == "i32" else "_wide"
        comb = {"i32": "i32.sub", "i64": "i64.sub", "f64": "f64.copysign", "v128": "i64x2.sub"}[t]
        if self.r.random() < 0.5:
            self.tag("stale", "tee" + wide)
            return ["local.get " + x] + self.val(t) + ["local.tee " + x, comb] + self.sink(t)
        self.tag("stale", "set" + wide)
        t2 = self.ty()
        return ["local.get " + x] + self.val(t2) + self.val(t) + ["local.set " + x] + self.sink(t2) + \
            ["local.get " + x, comb] + self.sink(t)

    def k_retarget(self, depth, long_run=None):
        """a producer that is local.set's source: directly after a label (not retargetable),
        after folded instructions (their count moves into the producer's cnt and post)"""
        kind = "nops" if long_run else self.pick("retarget", ["label", "nops", "const_label", "const_nops"])
        self.tag("retarget", kind)
        t = self.pick("rt", ["i32", "i64", "i32"])
        x = self.local(t, write=True)
        prod = ["%s.const %d" % (t, self.r.randrange(1000))] if kind.startswith("const") else \
            ["local.get " + self.local(t), "local.get " + self.local(t), t + ".add"]
        if kind.endswith("label"):
            mid = self.r.choice([["block", "end"], ["loop", "end"], ["block"] + self.simple() + ["end"]])
        elif long_run:
            mid = self.run("retarget", long_run)
        else:
            mid = self.run("retarget", self.r.choice([2, 2, 126, 254]) if self.seed % 4 == 1 else 2)
        return prod + mid + ["local.set " + x]

    def k_run(self, depth, long_run=None):
        pos = long_run[0] if long_run else self.pick("runpos", ["label", "branch", "loop"])
        n = long_run[1] if long_run else None
        if pos == "loop":
            return self.k_loop(depth, n or self.pick("runlen", [3]))
        if pos == "label":        # the store leaves nothing pending: the run is all that is
            return ["block"] + self.store() + self.run("label", n) + ["end"]
        return ["block"] + self.cond(2) + ["br_if 0"] + self.run("branch", n) + ["end"]

    def k_deadlabel(self, depth):
        """$x: only a dead br reaches it; $y: nothing does; what follows them never runs"""
        self.tag("label", "dead_only")
        self.tag("label", "unreached")
        return ["block"] + self.cond(2) + ["if", "block", "br 2", "br 0", "end"] + self.simple() + \
            ["block", "i32.const 7", "local.set $a", "br 2", "end"] + self.simple() + ["end", "end"]

    def stmt(self, depth):
        if depth >= MAXD or self.budget <= 0:
            return self.simple() if self.r.random() < 0.7 else self.store()
        self.budget -= 1
        k = self.pick("stmt", ["simple", "store", "block", "nest", "loop", "block", "nest", "call", "stale",
                               "retarget", "run", "simple", "nest", "block", "deadlabel", "return"])
        if k == "simple":
            return self.simple()
        if k == "store":
            return self.store()
        return getattr(self, "k_" + k)(depth)

    # ---- functions
    LOCALS = "(local $a i32) (local $b i32) (local $t i32) (local $fuel i32) (local $q i64) (local $f f64) (local $v v128)"

    def function(self, fn, must, extra):
        """`must`: statement kinds every function of this name gets, in a shuffled order with
        `extra` deck statements between them"""
        self.fn = fn
        self.labels = [("func", ["i64"])]
        self.budget = extra + len(must)
        r = self.r
        out = ["i32.const %d" % FUEL[fn], "local.set $fuel"]
        if fn == "rec":      # the depth: at most 12, whatever the caller passed
            out += ["local.get $p", "i64.const 15", "i64.and", "local.tee $p", "i64.const 12", "local.get $p",
                    "i64.const 12", "i64.lt_u", "select", "local.set $p"]
        out += self.lane(0xFFFF) + ["local.set $a", "local.get $s", "i32.const %d" % r.randrange(1 << 30), "i32.xor",
                                    "local.set $b", "local.get $s", "i64.extend_i32_u",
                                    "i64.const %d" % (r.randrange(1 << 40) * 2 + 1), "i64.mul", "local.set $q",
                                    "local.get $a", "f64.convert_i32_s", "local.set $f",
                                    "local.get $b", "i32x4.splat", "local.set $v"]
        if fn == "run":
            out += ["local.get $q", "i64.const 17", "i64.rotl", "local.set $p"]
        todo = list(must) + [None] * extra
        r.shuffle(todo)
        for k in todo:
            if k is None:
                out += self.stmt(1)
            elif isinstance(k, tuple):
                out += getattr(self, "k_" + k[0])(1, k[1])
            else:
                out += getattr(self, "k_" + k)(1)
        if fn == "rec":
            j, jt = self.junk()
            out += ["local.get $p", "i64.eqz", "i32.eqz", "if"] + j + ["block (result i64)"] + self.sarg() + \
                ["local.get $p", "i64.const 1", "i64.sub", "call $rec", "end", "local.get $q", "i64.const 1",
                 "i64.rotl", "i64.xor", "local.set $q"] + ["drop"] * len(jt) + ["end"]
        if fn == "run":
            out += ["i32.const 0", "local.get $a", "i32.store offset=%d" % FINAL,
                    "i32.const 0", "local.get $b", "i32.store offset=%d" % (FINAL + 4),
                    "i32.const 0", "local.get $p", "i64.store offset=%d" % (FINAL + 8),
                    "i32.const 0", "local.get $q", "i64.store offset=%d" % (FINAL + 16),
                    "i32.const 0", "local.get $f", "f64.store offset=%d" % (FINAL + 24),
                    "i32.const 0", "local.get $v", "v128.store offset=%d" % (FINAL + 32),
                    "i32.const 0", "local.get $fuel", "i32.store offset=%d" % (FINAL + 48)]
        out += ["local.get $p", "local.get $q", "i64.const 13", "i64.rotl", "i64.xor",
                "local.get $a", "i64.extend_i32_u", "i64.add", "local.get $b", "i64.extend_i32_u", "i64.const 32",
                "i64.shl", "i64.xor", "local.get $f", "i64.reinterpret_f64", "i64.add",
                "local.get $v", "i64x2.extract_lane 0", "i64.xor", "local.get $v", "i64x2.extract_lane 1", "i64.add"]
        assert len(self.labels) == 1
        head = "(func $%s%s (param $s i32) %s (result i64) %s%s" % (
            fn, ' (export "run")' if fn == "run" else "", "" if fn == "run" else "(param $p i64)",
            "(local $p i64) " if fn == "run" else "", self.LOCALS)
        return head + "\n    " + "\n    ".join(out) + ")"


def generate(seed, tail=False, runs=True):
    """(text, generator): the generator holds the construct tags and the br_table sizes"""
    g = _Gen(seed, tail, runs)
    long_run = LONG_RUNS[seed % 8]
    where = {"label": "run", "branch": "run", "loop": "loop", "retarget": "retarget"}[long_run[0]]
    funcs = [g.function("h0", ["nest"], 1),
             g.function("rec", ["nest"], 0),
             g.function("h1", ["loopret", "call"], 1),
             g.function("h2", ["call", "block", "return"], 0)]
    lr = [(where, long_run[1]) if where != "run" else ("run", long_run)]
    if seed % 8 in LONGER_RUNS:
        lr.append(("run", LONGER_RUNS[seed % 8]))
    funcs.append(g.function("run", ["nest", "nest", "block", "loop", "return", "trap", "trap", ("call", "rec"), "indirect",
                                    "stale", "retarget", "run", "deadlabel"] + lr, 3))
    text = """(module
  (type $h (func (param i32 i64) (result i64)))
  (memory 1)
  (table 6 funcref)
  (elem (i32.const 0) %s)
  (func $w (param i32) (result i32) (local.get 0))
  %s)
""" % (" ".join(TABLE), "\n  ".join(funcs))
    return text, g


def ctrl_wat(seed, tail=False, runs=True):
    return generate(seed, tail, runs)[0]


def ctrl_module(seed, tail=False, runs=True):
    return assemble(ctrl_wat(seed, tail, runs))


def constructs(seeds, tail=False):
    """the construct tags that the modules of `seeds` hold, pooled"""
    out = set()
    for s in seeds:
        out |= generate(s, tail)[1].cov
    return out


def tables(seed, tail=False):
    """per br_table of the module, in ARMS order: its number of entries before the default"""
    return generate(seed, tail)[1].tables
