#!/usr/bin/env python3
"""Which device functions differ between two builds?  For a change that must leave the gfx950 code as it is
(a refactor of the host side, a rename, a moved header): the objects (or libraries) of the same name in two
directories are disassembled - the amdgcn code object inside each offload bundle, `llvm-objdump -d
--symbolize-operands` - and compared function by function on instruction text and branch labels.  Addresses, raw
encodings and the padding between functions are left out, so a function that only moved is equal.

Functions are matched by demangled name with the argument-type spelling stripped
(`void fbstab_mpc_kernel<64, false>(fbk::MpcLayout, ...)` -> `fbstab_mpc_kernel<64, false>`): renaming a kernel's
argument types changes its symbol, not its code.  A name that two functions of one object share after stripping
(overloads) keeps its arguments.

Beside the instructions, the `.regs` files the Makefile writes next to the objects (register budget reports) are
compared where both directories have them.

usage: tools/diff_device_code.py PARENT_OBJDIR HEAD_OBJDIR [name.o ...]
       (default: every *.o the parent directory holds, e.g. fbstab_amd/csrc/build/libfbstab_hip)
exit status 0: every function of the parent is in the head with the same instructions; 1 otherwise."""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dpp_hazards import disassemble, functions  # noqa: E402

CXXFILT = "c++filt"  # (binutils, as check_vgpr_budget.py)


def strip_arguments(name):
    """`void ns::f<a, (b)1>(T, U<V>) [clone x]` -> `ns::f<a, (b)1>`: cut at the parenthesis that opens the
    argument list (the first one outside every template bracket), then drop the return type in front."""
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and i > 0 and not name[:i].endswith("operator"):
            if name[i:].startswith("(anonymous namespace)"):
                continue
            name = name[:i]
            break
    depth = 0
    for i in range(len(name) - 1, -1, -1):  # the return type: what precedes the last space outside brackets
        ch = name[i]
        if ch in ">)":
            depth += 1
        elif ch in "<(":
            depth -= 1
        elif ch == " " and depth == 0:
            return name[i + 1:]
    return name


def function_text(ins):
    """One function as text, its branch labels renumbered from 0 in the order they are defined: objdump counts
    labels through the whole object, so a function behind one that gained a branch would differ in nothing else."""
    number = {}
    for lab, _ in ins:
        if lab:
            number.setdefault(lab, f"L{len(number)}")
    relabel = lambda m: number.get(m.group(0), m.group(0))  # noqa: E731
    return "\n".join((number[lab] + ": " if lab else "") + re.sub(r"\bL\d+\b", relabel, text) for lab, text in ins)


def device_functions(path, tmp):
    """-> {key: instruction text of the function}, key = demangled name without its arguments."""
    fns = []
    for dis in disassemble(path, tmp):
        fns += functions(dis)
    if not fns:
        return {}
    full = subprocess.run([CXXFILT], input="\n".join(n for n, _ in fns), capture_output=True, text=True,
                          check=True).stdout.splitlines()
    short = [strip_arguments(n) for n in full]
    out = {}
    for (_, ins), f, k in zip(fns, full, short):
        key = k if short.count(k) == 1 else f
        out[key] = function_text(ins)
    return out


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    parent, head = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or sorted(os.path.basename(p) for p in glob.glob(os.path.join(parent, "*.o")))
    if not names:
        print(f"no objects in {parent}")
        return 2
    bad = 0
    for name in names:
        with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as th:
            a = device_functions(os.path.join(parent, name), tp)
            b = device_functions(os.path.join(head, name), th)
        if not a or not b:
            print(f"{name}: no amdgcn code object found in {'the parent' if not a else 'the head'} (nothing compared)")
            bad += 1
            continue
        gone = sorted(k for k in a if k not in b)
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        new = sorted(k for k in b if k not in a)
        for k in gone:
            print(f"{name}: MISSING in the head: {k}")
        for k in differ:
            la, lb = a[k].count("\n") + 1, b[k].count("\n") + 1
            print(f"{name}: DIFFERS: {k}  ({la} -> {lb} instructions)")
        for k in new:
            print(f"{name}: new in the head: {k}")
        regs = [os.path.join(d, name + ".regs") for d in (parent, head)]
        regs_note = ""
        if all(os.path.exists(r) for r in regs):
            # (the reports print the symbols' demangled names: compare them without the argument types too)
            ra, rb = ([re.sub(r"\s+", " ", re.sub(r"\((?:[^()]|\([^()]*\))*\)\s+regs", " regs", line)).strip()
                       for line in open(r)] for r in regs)
            same = ra == rb
            regs_note = "; .regs equal" if same else "; .regs DIFFER"
            bad += 0 if same else 1
        print(f"{name}: {len(a)} functions in the parent, {len(a) - len(gone) - len(differ)} identical in the head, "
              f"{len(differ)} differ, {len(gone)} missing, {len(new)} new{regs_note}")
        bad += len(gone) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
