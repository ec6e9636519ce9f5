"""Seeded random modules of float and SIMD code for the compiled-run parity tests
(tests/test_float_random.py; DESIGN.md "Parity tests").

tests/test_jit.py's generator is integer-only. This one emits typed f32, f64 and v128 code
whose NaNs travel: through chains of results, through destinations that alias a source,
across both arms of a divergent branch, loop back edges, a call, a br_table and a trap,
into every kind of consumer that jit.cpp's nan_observable tells apart.

float_module(seed, mix) -> wasm bytes; float_wat(seed, mix) -> the text.

  mix "compiled"  only ops the compiled runs emit (COMPILED_OPS): runs are long, and their
                  scheduling, forwarding and folding span float ops
  mix "mixed"     adds the ops that end a run or leave the core (MIXED_OPS): NaNs cross the
                  boundary between the core and the C++ step in both directions

Frame: four locals each of f32 ($x), f64 ($y), v128 ($v) and i32 ($i), an i64 accumulator,
two loop counters; mutable f32, f64 and v128 globals. About 40 cells, far below the V
frames' limit, so the compiled runs are in use.

Operands: data segments hold the f32 and f64 tables of scalar_cases.TABLES and the vectors
of simd_cases.SPECIAL. The export's one i32 parameter $s is a per-lane seed the body never
overwrites; "refresh" statements reload a local from a table at (s * odd constant) >> 20,
masked (v128 values are also read 16 bytes at a time out of the scalar tables). Without
them the lanes' values collapse to a few NaNs and infinities after some tens of statements.

Memory (one page): tables at TAB_F32/TAB_F64/TAB_V, random stores into SCRATCH..SCRATCH+4K,
the final value of every local at FINAL. A few accesses sit at the page end (0x88 on some
lanes, a 16-byte access that straddles the end) under a lane-bit guard; one statement per
module may trap with 0x84/0x85/0x86 (an i32/i64.trunc_f*, or an integer division by a
truncated float), under a lane-bit guard and right after a global.set and a store, so that
the state a trap leaves behind is compared too.

Exports: run(s) -> i64, and the getters g32() -> i32, g64() -> i64, gv() -> v128 that
return the globals' bits; rung(s) runs run(s) and folds the globals it leaves into an i64."""
import random

import scalar_cases
import simd_cases
from wasmedge_amd.wat import assemble

NLOC = 4
TAB_F32, TAB_F64, TAB_V = 0x100, 0x180, 0x280     # 32 x 4, 32 x 8, 16 x 16 bytes, contiguous
SCRATCH = 0x1000
FINAL = 0x8000      # x0..3 (4 bytes each), then y0..3 at +16, v0..3 at +48, i0..3 at +112
FINAL_F32, FINAL_F64, FINAL_V = FINAL, FINAL + 16, FINAL + 48

FCMP = ["eq", "ne", "lt", "gt", "le", "ge"]
_FT = ("f32", "f64")
_FV = ("f32x4", "f64x2")

COMPILED_OPS = sorted(
    ["%s.%s" % (t, o) for t in _FT for o in ["add", "sub", "mul", "abs", "neg", "copysign",
                                              "convert_i32_s", "convert_i32_u", "load", "store",
                                              "const"] + FCMP] +
    ["%s.%s" % (t, o) for t in _FV for o in ["add", "sub", "mul", "splat", "extract_lane",
                                              "replace_lane"] + FCMP] +
    ["%s.%s" % (t, o) for t in ("i32x4", "i64x2") for o in ["add", "sub", "shl", "shr_s", "shr_u",
                                                             "splat", "extract_lane", "replace_lane"]] +
    ["v128.and", "v128.or", "v128.xor", "v128.bitselect", "v128.any_true", "v128.const",
     "v128.load", "v128.store", "i32x4.bitmask", "select", "global.set", "global.get", "call",
     "br_table", "i32.reinterpret_f32", "i64.reinterpret_f64", "f32.reinterpret_i32",
     "f64.reinterpret_i64"])

_VUN = ["abs", "neg", "sqrt", "ceil", "floor", "trunc", "nearest"]
_NARROW_CMP = ["eq", "ne", "lt_s", "gt_s", "le_s", "ge_s"]
MIXED_OPS = sorted(
    ["%s.%s" % (t, o) for t in _FT for o in ["div", "min", "max", "sqrt", "ceil", "floor", "trunc",
                                              "nearest", "convert_i64_s", "convert_i64_u"]] +
    ["f64.promote_f32", "f32.demote_f64"] +
    ["%s.trunc_sat_%s_%s" % (i, f, s) for i in ("i32", "i64") for f in _FT for s in "su"] +
    ["%s.%s" % (t, o) for t in _FV for o in ["pmin", "pmax", "div", "min", "max"] + _VUN] +
    ["v128.andnot"] +
    ["%s.%s" % (t, o) for t in ("i8x16", "i16x8") for o in ["add", "sub"] + _NARROW_CMP] +
    ["%s.all_true" % t for t in ("i8x16", "i16x8", "i32x4", "i64x2")])

# the statement that may trap: i32/i64.trunc_f* (0x85, 0x86) or a division by one (0x84 too)
TRAP_OPS = ["%s.trunc_%s_%s" % (i, f, s) for i in ("i32", "i64") for f in _FT for s in "su"]

_F32_CONSTS = ["0", "-0", "1", "-1.5", "0.5", "inf", "-inf", "nan", "-nan", "nan:0x200001",
               "-nan:0x1234", "3.4028234e38", "1e-45", "16777216"]
_F64_CONSTS = ["0", "-0", "1", "-2.5", "0.5", "inf", "-inf", "nan", "-nan", "nan:0x4000000000001",
               "-nan:0x123456789", "1.7976931348623157e308", "5e-324", "1e300"]


class _Gen:
    def __init__(self, seed, mix, helper=False):
        assert mix in ("compiled", "mixed")
        self.r = random.Random("%s/%d/%d" % (mix, seed, helper))
        self.mix = mix
        self.seed = seed
        self.helper = helper      # the helper's body: no calls, no control flow, no traps
        self.labels = 0
        self.decks = {}

    # ---- operands
    def x(self):
        return "(local.get $x%d)" % self.r.randrange(NLOC)

    def y(self):
        return "(local.get $y%d)" % self.r.randrange(NLOC)

    def v(self):
        return "(local.get $v%d)" % self.r.randrange(NLOC)

    def i(self):
        return "(local.get $i%d)" % self.r.randrange(NLOC)

    def get(self, t):
        return {"f32": self.x, "f64": self.y, "v128": self.v, "i32": self.i}[t]()

    def dst(self, t):
        return "$%s%d" % ({"f32": "x", "f64": "y", "v128": "v", "i32": "i"}[t], self.r.randrange(NLOC))

    def lane_bits(self, mask):
        """some bits of the read-only seed, scrambled: (s * odd) >> 20, masked"""
        odd = self.r.randrange(1 << 31) * 2 + 1
        return "(i32.and (i32.shr_u (i32.mul (local.get $s) (i32.const %d)) (i32.const 20)) (i32.const %d))" \
            % (odd, mask)

    def fconst(self, t):
        return "(%s.const %s)" % (t, self.r.choice(_F32_CONSTS if t == "f32" else _F64_CONSTS))

    def table(self, t):
        """a fresh operand from the tables"""
        if t == "f32":
            return "(f32.load offset=%d %s)" % (TAB_F32, self.lane_bits(0x7C))
        if t == "f64":
            return "(f64.load offset=%d %s)" % (TAB_F64, self.lane_bits(0xF8))
        if t == "i32":
            return self.r.choice(["(i32.load offset=%d %s)" % (TAB_F32, self.lane_bits(0x7C)),
                                  self.lane_bits(self.r.choice([0x3F, 0xFFF, 0xFFFFFFFF]))])
        k = self.r.random()
        if k < 0.5:
            return "(v128.load offset=%d %s)" % (TAB_V, self.lane_bits(0xF0))
        if k < 0.9:    # 16 bytes of the scalar tables
            return "(v128.load offset=%d %s)" % (TAB_F32, self.lane_bits(0x170))
        return "(v128.load offset=%d %s)" % (TAB_F32, self.lane_bits(0x17C))    # (misaligned)

    def refresh(self, t=None):
        t = t or self.r.choice(["f32", "f64", "v128", "i32"])
        return "(local.set %s %s)" % (self.dst(t), self.table(t))

    def addr(self, n):
        """(address expression, offset) of an n-byte access into the scratch region: mostly
        aligned, sometimes not (the run leaves; the C++ step executes the access)"""
        if self.r.random() < 0.88:
            return self.lane_bits(0xFFF & ~(n - 1)), SCRATCH + self.r.choice([0, 0, 16, 32, 256])
        return self.lane_bits(0xFFF), SCRATCH + self.r.choice([0, 1, 2])

    # ---- expressions of a type (depth-limited: nested results live in stack temporaries,
    # never observable by themselves). Ops come off decks, so that the modules use every op of
    # their mix about equally often.
    def pick(self, key, items):
        """the next item of a deck: `items` in an order fixed per mix, walked cyclically from a
        start that depends on the seed, so that a set of seeds 0..7 covers a deck even where
        one module draws only an eighth of it"""
        if key not in self.decks:
            order = list(items)
            random.Random("%s/%s" % (self.mix, key)).shuffle(order)
            self.decks[key] = [order, (self.seed % 8) * len(order) // 8 + (len(order) // 16 if self.helper else 0)]
        d = self.decks[key]
        d[1] += 1
        return d[0][(d[1] - 1) % len(d[0])]

    def fbin_ops(self):
        return ["add", "sub", "mul", "copysign"] + (["div", "min", "max"] if self.mix == "mixed" else [])

    def fforms(self):
        f = ["add", "sub", "mul"] * 3 + ["copysign", "abs", "neg", "cvt_s", "cvt_u", "select", "lane", "bits"]
        if self.mix == "mixed":
            f += ["div", "min", "max", "sqrt", "ceil", "floor", "trunc", "nearest", "cvt64_s", "cvt64_u", "resize"] * 2
        return f

    def fexpr(self, t, depth=1):
        r = self.r
        leaf = lambda: self.get(t) if r.random() < 0.85 else self.fconst(t)
        sub = (lambda: self.fexpr(t, depth - 1)) if depth > 0 and r.random() < 0.4 else leaf
        k = self.pick("f" + t, self.fforms())
        if k in ("add", "sub", "mul", "copysign", "div", "min", "max"):
            return "(%s.%s %s %s)" % (t, k, sub(), sub())
        if k in ("abs", "neg", "sqrt", "ceil", "floor", "trunc", "nearest"):
            return "(%s.%s %s)" % (t, k, sub())
        if k in ("cvt_s", "cvt_u"):
            return "(%s.convert_i32_%s %s)" % (t, k[-1], self.i())
        if k in ("cvt64_s", "cvt64_u"):
            return "(%s.convert_i64_%s (local.get $acc))" % (t, k[-1])
        if k == "select":
            return "(select %s %s %s)" % (sub(), sub(), self.i())
        if k == "lane":
            sh, n = ("f32x4", 4) if t == "f32" else ("f64x2", 2)
            return "(%s.extract_lane %d %s)" % (sh, r.randrange(n), self.v())
        if k == "resize":
            return "(f32.demote_f64 %s)" % self.y() if t == "f32" else "(f64.promote_f32 %s)" % self.x()
        return "(%s.reinterpret_%s %s)" % ((t, "i32", self.i()) if t == "f32" else (t, "i64", "(local.get $acc)"))

    def vbin_ops(self):
        ops = ["%s.%s" % (s, o) for s in _FV for o in ["add", "sub", "mul"] * 2 + FCMP] + \
            ["v128.and", "v128.or", "v128.xor", "i32x4.add", "i32x4.sub", "i64x2.add", "i64x2.sub"]
        if self.mix == "mixed":
            ops += (["%s.%s" % (s, o) for s in _FV for o in ["pmin", "pmax", "div", "min", "max"]] +
                    ["v128.andnot"] +
                    ["%s.%s" % (s, o) for s in ("i8x16", "i16x8") for o in ["add", "sub"] + _NARROW_CMP]) * 2
        return ops

    def vbin(self):
        return self.pick("vbin", self.vbin_ops())

    def vforms(self):
        f = ["bin"] * 16 + ["shift"] * 5 + ["bitselect"] * 2 + ["splat"] * 3 + ["replace"] * 4 + ["select", "const"]
        return f + (["un"] * 12 if self.mix == "mixed" else [])

    def vexpr(self, depth=1):
        r = self.r
        sub = (lambda: self.vexpr(depth - 1)) if depth > 0 and r.random() < 0.35 else self.v
        k = self.pick("v", self.vforms())
        if k == "bin":
            return "(%s %s %s)" % (self.vbin(), sub(), sub())
        if k == "shift":
            op = self.pick("vsh", ["%s.%s" % (s, o) for s in ("i32x4", "i64x2") for o in ("shl", "shr_s", "shr_u")])
            return "(%s %s %s)" % (op, sub(), r.choice([self.i(), "(i32.const %d)" % r.choice([0, 1, 31, 33, 63])]))
        if k == "bitselect":
            return "(v128.bitselect %s %s %s)" % (sub(), sub(), self.v())
        if k == "splat":
            return self.pick("vsp", ["(f32x4.splat %s)" % self.x(), "(f64x2.splat %s)" % self.y(),
                                     "(i32x4.splat %s)" % self.i(), "(i64x2.splat (local.get $acc))"])
        if k == "replace":
            sh, n, e = self.pick("vrp", [("f32x4", 4, self.x()), ("f64x2", 2, self.y()), ("i32x4", 4, self.i()),
                                         ("i64x2", 2, "(local.get $acc)")])
            return "(%s.replace_lane %d %s %s)" % (sh, r.randrange(n), sub(), e)
        if k == "select":
            return "(select %s %s %s)" % (sub(), sub(), self.i())
        if k == "const":
            return r.choice(["(v128.const i32x4 0x7fc00001 0xffa00002 0x7f800000 0x3f800000)",
                             "(v128.const f64x2 -nan:0x8000000000123 inf)",
                             "(v128.const f32x4 1 -0 nan:0x200001 -inf)",
                             "(v128.const i64x2 -1 0x7ff0000000000001)"])
        return "(%s %s)" % (self.pick("vun", ["%s.%s" % (s, o) for s in _FV for o in _VUN]), sub())

    def vcmp(self):
        return "(%s %s %s)" % (self.pick("vcmp", ["%s.%s" % (s, o) for s in _FV for o in FCMP]),
                               self.vexpr(0), self.vexpr(0))

    def cond(self):
        """an i32 from a hidden consumer: a float compare, a trunc_sat (mixed), or the C5
        idiom -- any_true / all_true / bitmask of a vector compare"""
        r = self.r
        forms = ["fcmp"] * 6 + ["any"] * 3 + ["bitmask"] * 2 + ["anyv"]
        if self.mix == "mixed":
            forms += ["all"] * 4 + ["sat"] * 4
        k = self.pick("cond", forms)
        if k == "fcmp":
            op = self.pick("fcmp", ["%s.%s" % (t, o) for t in _FT for o in FCMP])
            return "(%s %s %s)" % (op, self.fexpr(op[:3]), self.fexpr(op[:3], 0))
        if k == "any":
            return "(v128.any_true %s)" % self.vcmp()
        if k == "bitmask":
            return "(i32.and (i32x4.bitmask %s) (i32.const %d))" % (self.vcmp(), r.choice([1, 2, 5, 8, 15]))
        if k == "anyv":
            return "(v128.any_true %s)" % self.v()
        if k == "all":
            return "(%s.all_true %s)" % (self.pick("all", ["i8x16", "i16x8", "i32x4", "i64x2"]), self.vcmp())
        op = self.pick("sat", ["%s.trunc_sat_%s_%s" % (i, f, s) for i in ("i32", "i64") for f in _FT for s in "su"])
        e = "(%s %s)" % (op, self.fexpr(op[14:17], 0))
        return "(i32.and %s (i32.const 1))" % e if op[:3] == "i32" else "(i64.eqz %s)" % e

    # ---- statements
    def alias(self):
        """x = x op y, x = y op x, x = x op x for a binary float or vector op"""
        r = self.r
        t = r.choice(["f32", "f64", "v128", "v128"])
        d = self.dst(t)
        dg, o = "(local.get %s)" % d, self.get(t)
        a, b = r.choice([(dg, o), (o, dg), (dg, dg)])
        if t == "v128":
            return "(local.set %s (%s %s %s))" % (d, self.vbin(), a, b)
        return "(local.set %s (%s.%s %s %s))" % (d, t, self.pick("fb" + t, self.fbin_ops()), a, b)

    def val(self, t):
        """what a sink consumes: a local, or a result that nothing but this sink can observe"""
        if self.r.random() < 0.5:
            return self.get(t)
        return self.vexpr(0) if t == "v128" else self.fexpr(t, 0)

    def sink(self):
        r = self.r
        k = r.randrange(9 if not self.helper else 8)
        if k == 0:
            t = r.choice(["f32", "f64", "v128"])
            ad, off = self.addr({"f32": 4, "f64": 8, "v128": 16}[t])
            return "(%s.store offset=%d %s %s)" % (t, off, ad, self.val(t))
        if k == 1:    # towards the return value, as bits
            e = r.choice(["(i64.reinterpret_f64 %s)" % self.val("f64"),
                          "(i64.extend_i32_u (i32.reinterpret_f32 %s))" % self.val("f32"),
                          "(i64x2.extract_lane %d %s)" % (r.randrange(2), self.val("v128"))])
            return "(local.set $acc (i64.xor (i64.rotl (local.get $acc) (i64.const 7)) %s))" % e
        if k == 2:
            t = r.choice(["f32", "f64", "v128"])
            g = {"f32": "$g32", "f64": "$g64", "v128": "$gv"}[t]
            if r.random() < 0.25:
                return "(local.set %s (global.get %s))" % (self.dst(t), g)
            return "(global.set %s %s)" % (g, self.val(t))
        if k == 3:    # a bit-level reader
            return r.choice(["(local.set %s (i32.reinterpret_f32 %s))" % (self.dst("i32"), self.x()),
                             "(local.set %s (i32x4.extract_lane %d %s))" % (self.dst("i32"), r.randrange(4), self.v()),
                             "(local.set %s (v128.xor %s %s))" % (self.dst("v128"), self.v(), self.v()),
                             "(local.set %s (i32.wrap_i64 (i64.shr_u (i64.reinterpret_f64 %s) (i64.const 29))))"
                             % (self.dst("i32"), self.y())])
        if k == 4:    # hidden consumers
            return "(local.set %s %s)" % (self.dst("i32"), self.cond())
        if k == 5:
            t = r.choice(["f32", "f64", "v128"])
            return "(local.set %s (select %s %s %s))" % (self.dst(t), self.get(t), self.get(t),
                                                       r.choice([self.i(), self.cond()]))
        if k == 6:    # a load back from the scratch region
            t = r.choice(["f32", "f64", "v128"])
            ad, off = self.addr({"f32": 4, "f64": 8, "v128": 16}[t])
            return "(local.set %s (%s.load offset=%d %s))" % (self.dst(t), t, off, ad)
        if k == 7:
            return "(local.set %s (i32.%s %s %s))" % (self.dst("i32"), r.choice(["add", "xor", "shr_u", "and"]),
                                                     self.i(), r.choice([self.i(), "(i32.const %d)" % r.choice([1, 3, 31])]))
        return self.call()

    def call(self):
        return "(local.set %s (call $h (local.get $s) %s %s %s))" % (self.dst("f64"), self.val("f32"), self.val("f64"),
                                                                    self.val("v128"))

    def skip(self):
        """a br_if on a hidden consumer, jumping over a few statements"""
        self.labels += 1
        lab = "$k%d" % self.labels
        return "(block %s (br_if %s %s) %s)" % (lab, lab, self.cond(),
                                               " ".join(self.stmt(False) for _ in range(self.r.randrange(1, 4))))

    def stmt(self, control=True):
        r = self.r
        k = r.random()
        if k < 0.15:
            return self.refresh()
        if k < 0.32:
            t = r.choice(_FT)
            return "(local.set %s %s)" % (self.dst(t), self.fexpr(t))
        if k < 0.47:
            return "(local.set %s %s)" % (self.dst("v128"), self.vexpr())
        if k < 0.57:
            return self.alias()
        if k < 0.61:    # plain copies and constants (MOV*, CONST*)
            t = r.choice(["f32", "f64", "v128"])
            if t == "v128":
                return "(local.set %s %s)" % (self.dst(t), r.choice([self.v(), "(v128.const f32x4 nan:0x1 -nan 0x1p-149 2)"]))
            return "(local.set %s %s)" % (self.dst(t), r.choice([self.get(t), self.fconst(t)]))
        if k < 0.69:    # hidden consumers
            return "(local.set %s %s)" % (self.dst("i32"), self.cond())
        if k < 0.76 and control and not self.helper:
            return self.skip()
        return self.sink()

    def unobserved(self):
        """products that only a compare reads, in stack temporaries that the next statement's
        load overwrites: nothing can observe their payloads, whatever else the module holds"""
        t = self.r.choice(_FT)
        return "(local.set %s (%s.%s (%s.mul %s %s) (%s.sub %s %s)))\n      (local.set %s %s)" % (
            self.dst("i32"), t, self.pick("ucmp", FCMP), t, self.get(t), self.get(t), t, self.get(t), self.get(t),
            self.dst("v128"), self.table("v128"))

    def block(self, n):
        return "\n      ".join(self.stmt() for _ in range(n))

    def page_end(self):
        """an access at the page end under a lane-bit guard: in bounds on some lanes, 0x88 on
        others, and (16 bytes) straddling the end"""
        r = self.r
        t, n = r.choice([("f32", 4), ("f64", 8), ("v128", 16), ("v128", 16)])
        ad = "(i32.add (i32.const %d) %s)" % (0x10000 - n - 4, self.lane_bits(0x1C if n == 16 else 0xC))
        acc = "(%s.store %s %s)" % (t, ad, self.get(t)) if r.random() < 0.5 else \
            "(local.set %s (%s.load %s))" % (self.dst(t), t, ad)
        return "(if (i32.eqz %s) (then %s))" % (self.lane_bits(0x1F), acc)

    def trap(self):
        """the module's one statement that may trap with 0x84/0x85/0x86, under a lane-bit guard,
        after a global.set and a store"""
        r = self.r
        op = r.choice(TRAP_OPS)
        it, ft = op[:3], op[10:13]
        src = r.choice([self.table(ft), self.table(ft), self.get(ft), "(%s.mul %s %s)" % (ft, self.get(ft), self.table(ft))])
        tr = "(%s %s)" % (op, src)
        if r.random() < 0.6:
            tr = "(%s.div_%s (%s.const 1000000) %s)" % (it, op[-1], it, tr)
        keep = "(local.set %s %s)" % (self.dst("i32"), tr) if it == "i32" else \
            "(local.set $acc (i64.add (local.get $acc) %s))" % tr
        gt = r.choice(["f32", "f64"])
        return "(if (i32.eqz %s) (then (global.set %s %s) (f64.store offset=%d %s %s) %s))" % (
            self.lane_bits(0x7), {"f32": "$g32", "f64": "$g64"}[gt], self.fexpr(gt, 0),
            SCRATCH, self.lane_bits(0xFF8), self.fexpr("f64", 0), keep)


def _data(at, blob):
    return '(data (i32.const %d) "%s")' % (at, "".join("\\%02x" % b for b in blob))


def _locals(skip0=False):
    out = []
    for p, t in (("x", "f32"), ("y", "f64"), ("v", "v128"), ("i", "i32")):
        out += ["(local $%s%d %s)" % (p, k, t) for k in range(1 if skip0 and p != "i" else 0, NLOC)]
    return " ".join(out) + " (local $acc i64)"


def float_wat(seed, mix="compiled", n=11):
    g = _Gen(seed, mix)
    h = _Gen(seed, mix, helper=True)
    r = g.r
    T = scalar_cases.TABLES
    data = [_data(TAB_F32, b"".join(v.to_bytes(4, "little") for v in T["f32"])),
            _data(TAB_F64, b"".join(v.to_bytes(8, "little") for v in T["f64"])),
            _data(TAB_V, b"".join(simd_cases.SPECIAL))]
    init = "\n    ".join("(local.set $%s%d %s)" % (p, k, g.table(t)) for p, t in
                         (("x", "f32"), ("y", "f64"), ("v", "v128"), ("i", "i32")) for k in range(NLOC))
    final = "\n    ".join(
        ["(f32.store offset=%d (i32.const 0) (local.get $x%d))" % (FINAL_F32 + 4 * k, k) for k in range(NLOC)] +
        ["(f64.store offset=%d (i32.const 0) (local.get $y%d))" % (FINAL_F64 + 8 * k, k) for k in range(NLOC)] +
        ["(v128.store offset=%d (i32.const 0) (local.get $v%d))" % (FINAL_V + 16 * k, k) for k in range(NLOC)] +
        ["(i32.store offset=%d (i32.const 0) (local.get $i%d))" % (FINAL_V + 64 + 4 * k, k) for k in range(NLOC)])
    # where the trap and the page-end accesses go: between two of the parts below
    extra = {}
    for s in [g.trap()] + [g.page_end() for _ in range(r.randrange(1, 3))]:
        extra.setdefault(r.randrange(2, 8), []).append(s)
    ex = lambda k: "\n    ".join(extra.get(k, []))
    esc_t = r.choice(_FT)
    esc = "(%s.%s %s %s)" % (esc_t, r.choice(["gt", "lt", "ge", "le"]), g.get(esc_t), g.fconst(esc_t))
    trips = r.randrange(2, 5)
    return """
(module
  (memory 1)
  (global $g32 (mut f32) (f32.const 1.5))
  (global $g64 (mut f64) (f64.const -nan:0x8000000000abc))
  (global $gv (mut v128) (v128.const f32x4 nan:0x200001 1 -inf -0))
  %s
  ;; the helper: float work on its arguments and on locals that start at zero
  (func $h (param $s i32) (param $x0 f32) (param $y0 f64) (param $v0 v128) (result f64)
    %s
    %s
    (f64.add (local.get $y%d) (f64x2.extract_lane 1 (f64x2.mul (local.get $v%d) (f64x2.splat (local.get $y0))))))
  (func $run (export "run") (param $s i32) (result i64)
    %s (local $n i32) (local $m i32)
    %s
    ;; straight line
    %s
    %s
    (if (i32.and (local.get $s) (i32.const 1))
      (then %s)
      (else %s))
    %s
    ;; counted trips: a lane-uniform constant trip count
    (loop $c
      %s
      (local.set $n (i32.add (local.get $n) (i32.const 1)))
      (br_if $c (i32.lt_u (local.get $n) (i32.const %d))))
    %s
    ;; a per-lane trip count
    (local.set $m (i32.add (i32.and (i32.shr_u (local.get $s) (i32.const 5)) (i32.const 3)) (i32.const 1)))
    (local.set $n (i32.const 0))
    (loop $p
      %s
      (local.set $n (i32.add (local.get $n) (i32.const 1)))
      (br_if $p (i32.lt_u (local.get $n) (local.get $m))))
    %s
    ;; an escape loop: out on a float compare, at most 8 trips
    (local.set $n (i32.const 0))
    (block $out
      (loop $e
        %s
        (br_if $out %s)
        (local.set $n (i32.add (local.get $n) (i32.const 1)))
        (br_if $e (i32.lt_u (local.get $n) (i32.const %d)))))
    %s
    (block $done (block $c3 (block $c2 (block $c1 (block $c0
      (br_table $c0 $c1 $c2 $c3 (i32.and (local.get $s) (i32.const 3))))
      %s (br $done))
      %s (br $done))
      %s (br $done))
      %s)
    %s
    %s
    %s
    %s
    (i64.xor (i64.xor (local.get $acc) (i64.reinterpret_f64 (local.get $y%d)))
             (i64.xor (i64.extend_i32_u (i32.reinterpret_f32 (local.get $x%d)))
                      (i64x2.extract_lane %d (local.get $v%d)))))
  ;; (for a runner that keeps no state between invocations: the globals a finished run leaves)
  (func (export "rung") (param $s i32) (result i64)
    (drop (call $run (local.get $s)))
    (i64.xor (i64.xor (i64.extend_i32_u (i32.reinterpret_f32 (global.get $g32)))
                      (i64.rotl (i64.reinterpret_f64 (global.get $g64)) (i64.const 13)))
             (i64.xor (i64x2.extract_lane 0 (global.get $gv))
                      (i64.rotl (i64x2.extract_lane 1 (global.get $gv)) (i64.const 29)))))
  (func (export "g32") (result i32) (i32.reinterpret_f32 (global.get $g32)))
  (func (export "g64") (result i64) (i64.reinterpret_f64 (global.get $g64)))
  (func (export "gv") (result v128) (global.get $gv)))
""" % ("\n  ".join(data),
       _locals(skip0=True), "\n    ".join(h.stmt(False) for _ in range(10)), r.randrange(NLOC), r.randrange(NLOC),
       _locals(), init,
       g.block(n // 2) + "\n      " + g.unobserved() + "\n      " + g.block(n - n // 2), ex(2),
       g.block(n), g.block(n), ex(3),
       g.block(n), trips, ex(4),
       g.block(n - 3), ex(5),
       g.block(5), esc, r.randrange(3, 9), ex(6),
       g.block(4), g.block(4), g.block(4), g.block(4), ex(7),
       g.call(), g.block(n), final,
       r.randrange(NLOC), r.randrange(NLOC), r.randrange(2), r.randrange(NLOC))


def float_module(seed, mix="compiled"):
    return assemble(float_wat(seed, mix))


def ops_covered(wats, names):
    """the op names of `names` that the texts use"""
    return {n for n in names if any("(%s " % n in w for w in wats)}
