#!/usr/bin/env python3
"""DPP read-after-VALU-write distances in a kernel's device assembly.

    python tools/dpp_hazard.py f.s <kernel-name-substring> [min_wait_states]

A DPP operand needs 2 wait states after the VALU instruction that wrote it (on gfx950 a
v_pk_fma_f32 result read by v_mov_b32_dpp one instruction later is wrong in some lanes:
profiles/r03/probe/pk_dpp_hazard.txt).  The compiler's hazard recognizer pads the
instructions it selects itself but does not see a packed op written as inline asm as the
writer, so this walks the assembly in program order and reports every DPP instruction whose
source VGPR was written fewer than min_wait_states (default 2) wait states earlier: any
instruction between the two counts 1, an `s_nop N` counts N + 1.  Labels and branches reset
nothing: the walk is over the straight-line text, which is the order every fall-through path
runs.  Exit status 1 when a short distance is found.
"""
import re
import sys

from loop_mix import kernel_lines

VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def regs(tok):
    out = []
    for m in VREG.finditer(tok):
        if m.group(1) is not None:
            out.append(int(m.group(1)))
        else:
            out.extend(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def scan(body, need=2):
    """[(line index, text, register, wait states)] of the DPP reads closer than `need`."""
    age = {}                                  # vgpr -> wait states since its last VALU write
    bad = []
    ndpp = 0
    for i, ln in enumerate(body):
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        op, _, rest = t.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if op.startswith("s_nop"):
            n = int(ops[0], 0) + 1
            for r in age:
                age[r] += n
            continue
        if op.startswith("v_") and "dpp" in op:
            ndpp += 1
            # the DPP operand is src0: the first source (v_fmac also reads its destination,
            # but not through the DPP path)
            for r in regs(ops[1].split()[0]):
                if age.get(r, 99) < need:
                    bad.append((i, t, r, age[r]))
        for r in age:
            age[r] += 1
        if op.startswith("v_") and not op.startswith("v_cmp") and ops:
            for r in regs(ops[0].split()[0]):
                age[r] = 0
    return bad, ndpp


def main():
    path, pat = sys.argv[1], sys.argv[2]
    need = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    name, body = kernel_lines(open(path).read().splitlines(), pat)
    bad, ndpp = scan(body, need)
    print(f"{name}: {ndpp} DPP instructions, {len(bad)} read a VGPR written < {need} wait states earlier")
    for i, t, r, a in bad[:20]:
        print(f"  line {i}: v{r} written {a} wait states before: {t}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
