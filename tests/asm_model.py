"""CPU model of the generated single-statement inline asm (fe25519_asm.h, p256_asm.h).

The two headers are read as text.  Every `asm volatile(...)` statement is parsed into its
instruction strings, its output / input / clobber lists and the `%N` operand mapping, checked
statically, and translated once into a Python function over integers that executes it for one
lane: 32-bit VGPRs, 64-bit register pairs, VCC as one bit.  Nothing here needs a GPU; the device
test (tests/test_gpu_hpke_edges.py) holds the model and the hardware bit-equal.

Static checks made while parsing (AsmModelError):
  * an unknown mnemonic, so a regenerated header cannot silently go unmodelled;
  * a fixed register (vN) written by the text but missing from the clobber list;
  * VCC written by the text but "vcc" missing from the clobber list;
  * an output operand that is not early-clobber ("=&").

Every run starts with the fixed registers, the outputs and VCC filled with garbage; `call` runs
each statement under two different fills and requires the same result, so no scratch register
is read before the statement writes it.

`call` also reports the VCC value consumed by the last v_cndmask of the statement: in all ten
routines that is the carry / borrow out of the first fold, i.e. whether the second, conditional
fold does anything.
"""
from __future__ import annotations

import os
import random
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "janus_amd", "csrc")
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

P25519 = 2**255 - 19


def edge_25519():
    """The 25519 edge operands (88 distinct values), loosely reduced in [0, 2^256)."""
    p = P25519
    e = [0, 1, 2, 18, 19, 20, 37, 38, 39, 75, 76, 77, p - 1, p, p + 1, 2 * p - 1, 2 * p,
         2 * p + 1, 2**255 - 1, 2**255, (p - 1) // 2, 2**224, 2**32 - 1, 2**128 - 1, 2**128,
         int("55" * 32, 16), int("aa" * 32, 16)]
    e += [2**256 - k for k in range(1, 65)]
    return list(dict.fromkeys(e))


class AsmModelError(Exception):
    pass


# mnemonic -> (destination kinds, source count); destination kinds: "d" one 32-bit register,
# "q" a 64-bit pair, "c" VCC.  A trailing "vcc" source (carry in) is counted as a source.
_ISA = {
    "v_mad_u64_u32": ("qc", 3),
    "v_add_co_u32": ("dc", 2),
    "v_addc_co_u32": ("dc", 3),
    "v_sub_co_u32": ("dc", 2),
    "v_subb_co_u32": ("dc", 3),
    "v_subbrev_co_u32": ("dc", 3),
    "v_add_u32": ("d", 2),
    "v_sub_u32": ("d", 2),
    "v_cndmask_b32_e64": ("d", 3),
    "v_mul_u32_u24": ("d", 2),
    "v_alignbit_b32": ("d", 3),
    "v_lshlrev_b32": ("d", 2),
    "v_and_b32": ("d", 2),
    "v_cmp_ne_u32": ("c", 2),
    "v_mov_b32": ("d", 1),
    "v_mov_b64": ("q", 1),
    "s_mov_b32": ("d", 1),
}

_OPERAND = re.compile(r'"([^"]*)"\s*\(([^()]*)\)')


def _split_operands(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


class Routine:
    """One parsed asm statement and its compiled one-lane executor."""

    def __init__(self, name, lines, outputs, inputs, clobbers):
        self.name = name
        self.outputs = outputs    # [(constraint, C expression)]
        self.inputs = inputs
        self.clobbers = clobbers
        self.insns = []
        for ln in lines:
            mn, _, rest = ln.strip().partition(" ")
            if mn not in _ISA:
                raise AsmModelError(f"{name}: unknown mnemonic {mn!r} in {ln!r}")
            ops = _split_operands(rest)
            dst, nsrc = _ISA[mn]
            if len(ops) != len(dst) + nsrc:
                raise AsmModelError(f"{name}: {ln!r}: {len(ops)} operands, expected "
                                    f"{len(dst) + nsrc}")
            self.insns.append((mn, ops))
        self.nops = len(outputs) + len(inputs)
        self._static_checks()
        self._compile()

    # ---- operands ---------------------------------------------------------------------
    def _reg(self, op):
        """Python variable name of a 32-bit register operand, or None for a literal."""
        m = re.fullmatch(r"%(\d+)", op)
        if m:
            if int(m.group(1)) >= self.nops:
                raise AsmModelError(f"{self.name}: operand {op} out of range")
            return f"o{m.group(1)}"
        m = re.fullmatch(r"v(\d+)", op)
        if m:
            return f"v{m.group(1)}"
        return None

    def _pair(self, op):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", op)
        if not m or int(m.group(2)) != int(m.group(1)) + 1:
            raise AsmModelError(f"{self.name}: bad 64-bit operand {op!r}")
        return f"v{m.group(1)}", f"v{m.group(2)}"

    def _src32(self, op):
        r = self._reg(op)
        if r:
            return r
        if op == "vcc":
            raise AsmModelError(f"{self.name}: vcc used as a 32-bit source")
        try:
            return str(int(op, 0) & M32)
        except ValueError:
            raise AsmModelError(f"{self.name}: bad operand {op!r}") from None

    def _src64(self, op):
        if op.startswith("v["):
            lo, hi = self._pair(op)
            return f"({lo} | {hi} << 32)"
        try:
            return str(int(op, 0) & M64)
        except ValueError:
            raise AsmModelError(f"{self.name}: bad 64-bit operand {op!r}") from None

    def _vcc_in(self, op, ln):
        if op != "vcc":
            raise AsmModelError(f"{self.name}: {ln}: carry-in must be vcc, is {op!r}")

    # ---- static checks ----------------------------------------------------------------
    def _static_checks(self):
        for i, (c, _) in enumerate(self.outputs):
            if not c.startswith("=&"):
                raise AsmModelError(f"{self.name}: output %{i} ({c!r}) is not early-clobber")
        for c, _ in self.inputs:
            if c not in ("v", "s"):
                raise AsmModelError(f"{self.name}: input constraint {c!r} not modelled")
        written, vcc_written = set(), False
        for mn, ops in self.insns:
            for kind, op in zip(_ISA[mn][0], ops):
                if kind == "c":
                    if op != "vcc":
                        raise AsmModelError(f"{self.name}: {mn}: carry-out must be vcc")
                    vcc_written = True
                elif kind == "q":
                    written.update(self._pair(op))
                else:
                    r = self._reg(op)
                    if r is None:
                        raise AsmModelError(f"{self.name}: {mn}: bad destination {op!r}")
                    m = re.fullmatch(r"%(\d+)", op)
                    if m and int(m.group(1)) >= len(self.outputs):
                        raise AsmModelError(f"{self.name}: {mn} writes input operand {op}")
                    if not m:
                        written.add(r)
        missing = sorted(written - set(self.clobbers), key=lambda r: int(r[1:]))
        if missing:
            raise AsmModelError(f"{self.name}: writes {missing} but the clobber list lacks them")
        if vcc_written and "vcc" not in self.clobbers:
            raise AsmModelError(f"{self.name}: writes vcc but the clobber list lacks it")
        self.fixed = sorted({c for c in self.clobbers if c != "vcc"} | written,
                            key=lambda r: int(r[1:]))

    # ---- translation to Python --------------------------------------------------------
    def _compile(self):
        no = len(self.outputs)
        body = []
        gi = 0
        for r in self.fixed + [f"o{i}" for i in range(no)]:
            body.append(f"{r} = g[{gi}]")
            gi += 1
        body.append(f"vcc = g[{gi}] & 1")
        self.ngarbage = gi + 1
        for i in range(len(self.inputs)):
            body.append(f"o{no + i} = x[{i}]")
        last_cnd = max((i for i, (mn, _) in enumerate(self.insns) if mn.startswith("v_cndmask")),
                       default=None)
        body.append("fold = 0")
        for i, (mn, ops) in enumerate(self.insns):
            ln = f"{mn} {', '.join(ops)}"
            s32, s64 = self._src32, self._src64
            if mn == "v_mad_u64_u32":
                lo, hi = self._pair(ops[0])
                body += [f"t = {s32(ops[2])} * {s32(ops[3])} + {s64(ops[4])}",
                         f"{lo} = t & {M32}", f"{hi} = t >> 32 & {M32}", "vcc = t >> 64"]
            elif mn in ("v_add_co_u32", "v_addc_co_u32"):
                cin = ""
                if mn == "v_addc_co_u32":
                    self._vcc_in(ops[4], ln)
                    cin = " + vcc"
                body += [f"t = {s32(ops[2])} + {s32(ops[3])}{cin}",
                         f"{self._reg(ops[0])} = t & {M32}", "vcc = t >> 32"]
            elif mn in ("v_sub_co_u32", "v_subb_co_u32", "v_subbrev_co_u32"):
                a, b = s32(ops[2]), s32(ops[3])
                if mn == "v_subbrev_co_u32":
                    a, b = b, a
                cin = ""
                if mn != "v_sub_co_u32":
                    self._vcc_in(ops[4], ln)
                    cin = " - vcc"
                body += [f"t = {a} - {b}{cin}", f"{self._reg(ops[0])} = t & {M32}",
                         "vcc = 1 if t < 0 else 0"]
            elif mn == "v_add_u32":
                body.append(f"{self._reg(ops[0])} = ({s32(ops[1])} + {s32(ops[2])}) & {M32}")
            elif mn == "v_sub_u32":
                body.append(f"{self._reg(ops[0])} = ({s32(ops[1])} - {s32(ops[2])}) & {M32}")
            elif mn == "v_cndmask_b32_e64":
                self._vcc_in(ops[3], ln)
                if i == last_cnd:
                    body.append("fold = vcc")
                body.append(f"{self._reg(ops[0])} = {s32(ops[2])} if vcc else {s32(ops[1])}")
            elif mn == "v_mul_u32_u24":
                body.append(f"{self._reg(ops[0])} = ({s32(ops[1])} & 0xffffff) * "
                            f"({s32(ops[2])} & 0xffffff) & {M32}")
            elif mn == "v_alignbit_b32":
                body.append(f"{self._reg(ops[0])} = ({s32(ops[1])} << 32 | {s32(ops[2])}) >> "
                            f"({s32(ops[3])} & 31) & {M32}")
            elif mn == "v_lshlrev_b32":
                body.append(f"{self._reg(ops[0])} = {s32(ops[2])} << ({s32(ops[1])} & 31) & {M32}")
            elif mn == "v_and_b32":
                body.append(f"{self._reg(ops[0])} = {s32(ops[1])} & {s32(ops[2])}")
            elif mn == "v_cmp_ne_u32":
                body.append(f"vcc = 1 if {s32(ops[1])} != {s32(ops[2])} else 0")
            elif mn in ("v_mov_b32", "s_mov_b32"):
                body.append(f"{self._reg(ops[0])} = {s32(ops[1])}")
            elif mn == "v_mov_b64":
                lo, hi = self._pair(ops[0])
                body += [f"t = {s64(ops[1])}", f"{lo} = t & {M32}", f"{hi} = t >> 32"]
            else:  # in _ISA but not translated: a gap in this file, not in the header
                raise AsmModelError(f"{self.name}: {mn} has no translation")
        body.append("return (" + ", ".join(f"o{i}" for i in range(no)) + ",), fold")
        src = "def run(x, g):\n" + "".join(f"    {b}\n" for b in body)
        ns = {}
        exec(compile(src, f"<asm model of {self.name}>", "exec"), ns)
        self.run = ns["run"]

    # ---- one call on integers ---------------------------------------------------------
    def _bind(self, vals):
        x = []
        for _, expr in self.inputs:
            m = re.fullmatch(r"(\w+)\.v\[(\d+)\]", expr)
            x.append(vals[m.group(1)] >> 32 * int(m.group(2)) & M32 if m else vals[expr] & M32)
        return x

    def call(self, a, b=0, k=0):
        """(result as an integer from r.v[0..7], VCC consumed by the last v_cndmask).  Runs
        under two garbage fills and requires both to agree."""
        x = self._bind({"a": a, "b": b, "k": k})
        res = []
        for g in self.fills():
            out, fold = self.run(x, g)
            r = 0
            for (_, expr), w in zip(self.outputs, out):
                m = re.fullmatch(r"r\.v\[(\d+)\]", expr)
                if m:
                    r |= w << 32 * int(m.group(1))
            res.append((r, fold))
        if res[0] != res[1]:
            raise AsmModelError(f"{self.name}: result depends on the initial register contents "
                                f"(a={a:#x} b={b:#x}): {res[0][0]:#x} / {res[1][0]:#x}")
        return res[0]

    def fills(self):
        if not hasattr(self, "_fills"):
            rnd = random.Random(self.name)
            f0 = [rnd.getrandbits(32) for _ in range(self.ngarbage)]
            f1 = [~v & M32 for v in f0]   # every bit differs, VCC included
            self._fills = (f0, f1)
        return self._fills


def parse_header(path):
    """{routine name: Routine} for every asm statement of a generated header."""
    text = open(path).read()
    routines = {}
    for m in re.finditer(r"DEV\s+\w+\s+(\w+)\s*\([^)]*\)\s*\{(.*?)\n\}", text, re.S):
        name, body = m.group(1), m.group(2)
        a = re.search(r"asm volatile\((.*?)\);", body, re.S)
        if not a:
            raise AsmModelError(f"{name}: no asm statement")
        parts = re.split(r"\n\s*:", a.group(1))
        if len(parts) != 4:
            raise AsmModelError(f"{name}: expected text : outputs : inputs : clobbers")
        lines = []
        for s in re.findall(r'"((?:[^"\\]|\\.)*)"', parts[0]):
            if not s.endswith("\\n\\t"):
                raise AsmModelError(f"{name}: instruction string {s!r} lacks its line end")
            lines.append(s[:-4])
        outputs = _OPERAND.findall(parts[1])
        inputs = _OPERAND.findall(parts[2])
        clobbers = re.findall(r'"([^"]*)"', parts[3])
        if not lines or not outputs:
            raise AsmModelError(f"{name}: empty asm statement")
        routines[name] = Routine(name, lines, outputs, inputs, clobbers)
    if not routines:
        raise AsmModelError(f"{path}: no routine found")
    return routines


_cache = {}


def load(header):
    """parse_header of a header under janus_amd/csrc (by file name) or at a path, cached."""
    path = header if os.path.sep in header else os.path.join(CSRC, header)
    key = (os.path.abspath(path), os.path.getmtime(path))
    if key not in _cache:
        _cache[key] = parse_header(path)
    return _cache[key]


# ---- the shared 25519 operands and their model results (tests, CPU and GPU) -------------------
FE_OPS = ["fe_mul", "fe_sqr", "fe_add", "fe_sub", "fe_mul121665"]
FE_PY = [lambda x, y: x * y, lambda x, y: x * x, lambda x, y: x + y, lambda x, y: x - y,
         lambda x, y: 121665 * x]


def operands_25519(n_random=4096, seed=25519):
    """(a, b, number of edge pairs): the full edge x edge cross product, then random pairs."""
    e = edge_25519()
    rnd = random.Random(seed)
    a = [x for x in e for _ in e]
    b = [y for _ in e for y in e]
    ne = len(a)
    a += [rnd.randrange(2**256) for _ in range(n_random)]
    b += [rnd.randrange(2**256) for _ in range(n_random)]
    return a, b, ne


def model_25519(op):
    """[(result, fold taken)] of routine FE_OPS[op] over operands_25519(), computed once."""
    key = ("model_25519", op)
    if key not in _cache:
        r = load("fe25519_asm.h")[FE_OPS[op]]
        a, b, _ = operands_25519()
        _cache[key] = [r.call(x, y) for x, y in zip(a, b)]
    return _cache[key]
