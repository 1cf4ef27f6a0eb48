"""Load-to-use distance of the global loads of a kernel's multiply loops, from gfx950 assembly.

Usage: python tools/isa_load_use.py --asm FILE.s --kernel MANGLED_NAME_OR_SUBSTRING [--min-mads N]

The assembly comes from
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
        -o FILE.s janus_amd/csrc/prio3_prepare.hip

For every kernel whose mangled name contains --kernel it prints

1. each single-block loop (a label, no other label up to a branch back to it) that holds both a
   `global_load` and a `v_mad_u64_u32`: per load, the loaded registers, the first instruction
   that reads one of them (taken cyclically around the loop: a value loaded in one trip may be
   read in the next) and how many `v_mad_u64_u32` lie between the two.  A load whose first reader
   is fewer than --min-mads (default 64, one trip of a two-wire sweep) multiplies behind it is
   marked SHORT: a wave reaches that reader long before an L2 miss can have come back.

2. every `global_load` of the kernel that is waited for at once: the first `s_waitcnt vmcnt(k)`
   that covers it comes after at most --near (default 4) vector or memory instructions; with
   --near 0 only scalar instructions may lie between the load and an `s_waitcnt vmcnt(0)`.  That
   is a fully exposed round trip.  (The compiler likes to put the next address computation
   between a load and its wait, so the strict rule misses most of them.)  They are listed with
   the basic block and counted per enclosing loop header, so "how many exposed waits does one
   sweep of the wire loop pay" is the count under the header of the loop around the multiply
   loop.

The exit status is 1 if a multiply loop of at least --min-mads multiplies has a SHORT load,
else 0.  Plain text in, plain text out: nothing is compiled or run here.
"""
from __future__ import annotations

import argparse
import re
import sys
from collections import Counter

STORE = re.compile(r"^(global_store|scratch_store|flat_store|buffer_store|ds_write|ds_store|"
                   r"global_atomic|flat_atomic|ds_add|ds_max|ds_min)")
LABEL = re.compile(r"^(\.LBB\w+):")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def split_kernels(lines):
    kern, cur = {}, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):\s*;\s*@", ln)
        if m:
            cur = m.group(1)
            kern[cur] = []
            continue
        if cur and ln.startswith(".Lfunc_end"):
            cur = None
        if cur is not None:
            kern[cur].append(ln)
    return kern


def vregs(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def parse(ln):
    """(mnemonic, written VGPRs, read VGPRs) of one assembly line, or None for a non-instruction."""
    s = ln.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    op, _, rest = s.partition(" ")
    ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
    if not ops:
        return op, set(), set()
    if STORE.match(op):
        return op, set(), vregs(rest)
    # everything else: the first operand is written, the others are read (an accumulator that is
    # both, as in v_mad_u64_u32 or v_addc, appears again among the sources)
    return op, vregs(ops[0]), vregs(", ".join(ops[1:]))


def blocks(body):
    """[(label, loop comment, [(line number, text)])] in layout order."""
    out = [("entry", "", [])]
    for i, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            out.append((m.group(1), ln.split(";", 1)[1].strip() if ";" in ln else "", []))
            continue
        s = ln.strip()
        if s.startswith(";") and not out[-1][2]:  # LLVM's loop comments under the label
            out[-1] = (out[-1][0], (out[-1][1] + " " + s.lstrip("; ")).strip(), out[-1][2])
            continue
        if parse(ln) is not None:
            out[-1][2].append((i + 1, s.split(";")[0].strip()))
    return out


def enclosing(comment, label):
    """The header of the innermost loop a block belongs to, from LLVM's block comment."""
    if "Loop Header" in comment:
        return label.lstrip(".L")
    m = re.search(r"in Loop: Header=(BB\w+)", comment)
    if m:
        return m.group(1)
    m = re.findall(r"Parent Loop (BB\w+)", comment)
    return m[-1] if m else "-"


def parent_of(comment):
    m = re.findall(r"Parent Loop (BB\w+)", comment)
    return m[-1] if m else "-"


def multiply_loops(blks, min_mads):
    short = 0
    for label, comment, ins in blks:
        if not ins:
            continue
        last = ins[-1][1]
        back = any(re.match(r"^s_cbranch\w*\s+" + re.escape(label) + r"$", t) or
                   re.match(r"^s_branch\s+" + re.escape(label) + r"$", t) for _, t in ins[-2:])
        nmad = sum(t.startswith("v_mad_u64_u32") for _, t in ins)
        nld = sum(t.startswith("global_load") for _, t in ins)
        if not back or not nmad or not nld:
            continue
        print(f"  multiply loop {label} (parent loop {parent_of(comment)}): {len(ins)} instructions, "
              f"{nmad} v_mad_u64_u32, {nld} global_load, ends `{last}`")
        n = len(ins)
        par = [parse(t) for _, t in ins]
        for i, (lno, t) in enumerate(ins):
            if not t.startswith("global_load"):
                continue
            dst = par[i][1]
            mads, reader = 0, None
            for step in range(1, n + 1):
                j = (i + step) % n
                op, wr, rd = par[j]
                if rd & dst:
                    reader = (ins[j][1], step, j < i or step == n)
                    break
                if op.startswith("v_mad_u64_u32"):
                    mads += 1
                dst = dst - wr  # overwritten before any read: that part of the load is dead
                if not dst:
                    break
            regs = t.split()[1].rstrip(",")
            if reader is None:
                print(f"    line {lno}: {regs:10s} no reader inside the loop")
                continue
            flag = "" if mads >= min_mads else "   SHORT"
            short += mads < min_mads and nmad >= min_mads
            print(f"    line {lno}: {regs:10s} {mads:3d} v_mad_u64_u32 before its first reader, "
                  f"{reader[1]} instructions on{' (next trip)' if reader[2] else ''}: "
                  f"`{reader[0]}`{flag}")
    return short


VMEM = re.compile(r"^(global_|scratch_|buffer_|flat_)")


def exposed_loads(blks, near):
    """Loads whose round trip is waited for at once: the first `s_waitcnt vmcnt(k)` that covers
    the load (k <= number of memory operations issued after it) comes after at most `near`
    vector or memory instructions.  near = 0 is the strict rule: only scalar instructions lie
    between the load and an `s_waitcnt vmcnt(0)`."""
    flat = [(label, comment, lno, t) for label, comment, ins in blks for lno, t in ins]
    per_loop, total = Counter(), 0
    for i, (label, comment, lno, t) in enumerate(flat):
        if not t.startswith("global_load"):
            continue
        later, vec = 0, 0
        for _, _, _, u in flat[i + 1:]:
            if u.startswith("s_waitcnt"):
                m = re.search(r"vmcnt\((\d+)\)", u)
                if m and int(m.group(1)) <= later:
                    hdr = enclosing(comment, label)
                    per_loop[hdr] += 1
                    total += 1
                    print(f"    line {lno}: `{t}` waited for by `{u}` after {vec} vector / memory "
                          f"instructions   block {label}, loop {hdr}")
                    break
                continue
            if u.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier", "s_setpc")):
                break
            if u.startswith("s_"):
                continue
            vec += 1
            later += bool(VMEM.match(u))
            if vec > near:
                break
    print(f"  exposed loads: {total}; per enclosing loop header: "
          + (", ".join(f"{k}: {v}" for k, v in sorted(per_loop.items())) or "none"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", required=True)
    ap.add_argument("--kernel", required=True)
    ap.add_argument("--min-mads", type=int, default=64)
    ap.add_argument("--near", type=int, default=4)
    a = ap.parse_args()
    kern = split_kernels(open(a.asm).read().splitlines())
    short, seen = 0, 0
    for k, body in kern.items():
        if a.kernel not in k:
            continue
        seen += 1
        print(k)
        blks = blocks(body)
        short += multiply_loops(blks, a.min_mads)
        print(f"  global loads waited for within {a.near} vector / memory instructions:")
        exposed_loads(blks, a.near)
    if not seen:
        sys.exit(f"no kernel matches {a.kernel!r}")
    sys.exit(1 if short else 0)


if __name__ == "__main__":
    main()
