#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel (the method profiles/threshold.md describes, as a tool).

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -I include --cuda-device-only -S -o old.s FILE.hip   # at one commit
    hipcc ... -o new.s FILE.hip                                                                             # at the other
    python tools/kernel_isa_diff.py old.s new.s [--map OLD=NEW ...] [--markdown]

A kernel is the lines from its label to its `.Lfunc_end`, comments stripped, the function number taken out of the
branch labels (`.LBB7_3` -> `.LBB_3`) and the kernel's own symbol replaced by a placeholder.  Kernels are paired by
their short name -- the demangled name without namespace and parameter list, spaces removed, e.g. `compose_fwd_kernel`
or `p_sample_tail_kernel<true,false,true>` -- and `--map OLD=NEW` pairs a renamed kernel with its predecessor.

One verdict per kernel:
  identical     the same lines.
  kernarg-only  the same number of lines, and the only lines that differ are scalar loads from the kernarg pointer that
                differ in nothing but their offset immediate, and `.amdhsa_kernarg_size`.
  differs       anything else; then the per-opcode count differences follow (and whether the vector / LDS / memory opcodes
                among them are the same multiset), with VGPR / SGPR / scratch / LDS from the `.amdhsa_*` lines of both.
Exit status 1 if a kernel of OLD has no partner in NEW, else 0: the verdicts are for a person (or a gate) to read.
"""
import argparse
import collections
import re
import subprocess
import sys

RESOURCES = (("VGPR", ".amdhsa_next_free_vgpr"), ("SGPR", ".amdhsa_next_free_sgpr"),
             ("scratch", ".amdhsa_private_segment_fixed_size"), ("LDS", ".amdhsa_group_segment_fixed_size"))
VECTOR_OR_MEMORY = ("v_", "ds_", "global_", "flat_", "buffer_", "scratch_")


def demangle(names):
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    except FileNotFoundError:                        # no binutils: the mangled names serve as they are
        out = names
    return dict(zip(names, out))


def short_name(demangled):
    s = demangled.replace("(anonymous namespace)::", "")
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):                       # the parameter list opens at the first '(' outside <...>
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut]
    if s.startswith("void "):
        s = s[5:]
    return s.replace(" ", "")


def kernels(path):
    """-> {short name: normalised lines} of every kernel (a symbol with an .amdhsa_kernel block) of a listing."""
    lines = open(path).read().splitlines()
    symbols = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    names = demangle(symbols)
    out = {}
    for sym in symbols:
        try:
            start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        except StopIteration:
            continue
        body = []
        for l in lines[start:]:
            l = l.split(";", 1)[0].rstrip()
            if not l.strip():
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", l).replace(sym, "<kernel>"))
            if re.match(r"\.Lfunc_end\d+:", l):
                body[-1] = ".Lfunc_end:"
                break
        out[short_name(names[sym])] = body
    return out


def kernarg_pointers(body):
    """The SGPR pairs that hold the kernarg pointer: s[0:1] as the launch leaves it, and plain copies of it."""
    regs = {"s[0:1]"}
    for l in body:
        m = re.match(r"\s*s_mov_b64\s+(s\[\d+:\d+\]),\s*(s\[\d+:\d+\])\s*$", l)
        if m and m.group(2) in regs:
            regs.add(m.group(1))
    return regs


def kernarg_only(a, b):
    if len(a) != len(b):
        return False
    ptrs = kernarg_pointers(a) & kernarg_pointers(b)
    load = re.compile(r"(\s*s_load_dword\w*\s+\S+,\s*(s\[\d+:\d+\]),\s*)(0x[0-9a-f]+|\d+)\s*$")
    for x, y in zip(a, b):
        if x == y:
            continue
        if x.split()[0] == y.split()[0] == ".amdhsa_kernarg_size":
            continue
        mx, my = load.match(x), load.match(y)
        if not (mx and my and mx.group(1) == my.group(1) and mx.group(2) in ptrs):
            return False
    return True


def opcodes(body):
    c = collections.Counter()
    for l in body:
        w = l.split()[0]
        if not w.startswith(".") and not w.endswith(":") and w != "<kernel>:":
            c[w] += 1
    return c


def resources(body):
    r = {}
    for key, directive in RESOURCES:
        r[key] = next((l.split()[1] for l in body if l.split()[0] == directive), "?")
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", nargs="+", action="extend", default=[], metavar="OLD=NEW",
                    help="pair kernel OLD of the first listing with kernel NEW of the second (short names)")
    ap.add_argument("--markdown", action="store_true", help="print the table as markdown")
    args = ap.parse_args(argv)
    old, new = kernels(args.old), kernels(args.new)
    pairs = dict(m.split("=", 1) for m in args.map)
    missing, used = [], set()
    rows, details = [], []
    for name, a in old.items():
        partner = pairs.get(name, name)
        b = new.get(partner)
        if b is None:
            missing.append(name)
            rows.append((name, partner, "no partner", len(a), 0))
            continue
        used.add(partner)
        if a == b:
            verdict = "identical"
        elif kernarg_only(a, b):
            verdict = "kernarg-only (%d lines)" % sum(x != y for x, y in zip(a, b))
        else:
            verdict = "differs"
            oa, ob = opcodes(a), opcodes(b)
            diff = {k: (oa[k], ob[k]) for k in sorted(set(oa) | set(ob)) if oa[k] != ob[k]}
            vm = [k for k in diff if k.startswith(VECTOR_OR_MEMORY)]
            ra, rb = resources(a), resources(b)
            details.append((name, partner, diff, vm, ra, rb))
        rows.append((name, partner, verdict, len(a), len(b)))
    for name, b in new.items():
        if name not in used:
            rows.append(("-", name, "new", 0, len(b)))
    if args.markdown:
        print("| kernel (old) | kernel (new) | lines old → new | verdict |\n|---|---|---|---|")
        for o, n, v, la, lb in rows:
            print(f"| `{o}` | {'=' if n == o else '`' + n + '`'} | {la} → {lb} | {v} |")
    else:
        for o, n, v, la, lb in rows:
            print(f"{o:52s} {'' if n == o else '-> ' + n:48s} {la:5d} -> {lb:5d}  {v}")
    for name, partner, diff, vm, ra, rb in details:
        print(f"\n{name} -> {partner}: differs")
        print("  " + "  ".join(f"{k} {ra[k]} / {rb[k]}" for k, _ in RESOURCES) + "   (old / new)")
        print("  vector, LDS and memory opcodes: " + ("the same multiset" if not vm else "DIFFERENT: " + ", ".join(vm)))
        print("  opcode counts that differ (old / new): " +
              (", ".join(f"{k} {x} / {y}" for k, (x, y) in diff.items()) or "none (the same opcodes in another order)"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
