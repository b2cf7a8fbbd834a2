#!/usr/bin/env python3
"""Are the kernels of two device assembly files the same?  CPU only.

    hipcc <the Makefile's CXXFLAGS> --offload-device-only -S a.hip -o OLD.s      (likewise NEW.s; several files: concatenate them)
    tools/kernel_isa_diff.py OLD.s NEW.s [--map old=new ...]

Per kernel symbol (every `.amdhsa_kernel NAME`) the function body (from the label `NAME:` to the descriptor) and the descriptor block
(`.amdhsa_kernel` .. `.end_amdhsa_kernel`: registers, LDS, scratch, kernarg size) are compared as text, after comments and `.loc` /
`.file` / `.cfi` lines are dropped, the kernel's own name is replaced and local labels (.LBB*, .Lfunc_end*, .Ltmp*) are numbered by
first appearance.  --map rewrites OLD's kernel names before they are matched (plain substring replacement, so one entry can map a
namespace prefix of every kernel); a renamed kernel that is not mapped shows up as present on one side only.  Prints one line per
kernel and exits 1 on any difference.  It compares text and knows no instruction."""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L(?:BB|func_end|tmp)[0-9_]+")
DROPPED = (".loc", ".file", ".cfi")


def normalised(lines, name):
    labels, out = {}, []
    for ln in lines:
        ln = ln.split(";", 1)[0].replace(name, "<kernel>").strip()
        if not ln or ln.startswith(DROPPED):
            continue
        out.append(LOCAL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln))
    return out


def kernels_of(path):
    """name -> (body, descriptor), both normalised"""
    lines = open(path).read().splitlines()
    found = {}
    for i, ln in enumerate(lines):
        if not ln.strip().startswith(".amdhsa_kernel "):
            continue
        name = ln.split()[1]
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        start = max(j for j in range(i) if lines[j].split(";", 1)[0].strip() == name + ":")
        found[name] = (normalised(lines[start:i], name), normalised(lines[i:end + 1], name))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", nargs="*", default=[], metavar="old=new", help="substring of OLD's kernel names and its replacement")
    args = ap.parse_args()
    old, new = kernels_of(args.old), kernels_of(args.new)
    for m in args.map:
        a, b = m.split("=", 1)
        old = {k.replace(a, b): v for k, v in old.items()}
    differ = 0
    for name in sorted(set(old) & set(new)):
        what = [w for w, o, n in zip(("body", "descriptor"), old[name], new[name]) if o != n]
        differ += bool(what)
        print(f"{'differs (' + ', '.join(what) + ')' if what else 'same':24s} {name}")
    only = [(side, k) for side, here, there in (("old", old, new), ("new", new, old)) for k in sorted(set(here) - set(there))]
    for side, k in only:
        print(f"{'only in ' + side:24s} {k}")
    print(f"{len(old)} kernels in old, {len(new)} in new: {len(set(old) & set(new)) - differ} same, {differ} differ, {len(only)} on one side only")
    return 1 if differ or only else 0


if __name__ == "__main__":
    sys.exit(main())
