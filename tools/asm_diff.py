#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two gfx950 assembly files of adac_kernels.hip (hipcc ... -save-temps=obj, as
`make asm` does, with the Makefile's KFLAGS): which kernels have the same machine code in both, which differ, which
exist on one side only.  A clean-up that may not touch a shipped kernel is checked with it on a machine without a GPU.

A kernel's text runs from its label to its .Lfunc_endN: the instructions and the .amdhsa_kernel descriptor.  Comments
are stripped and the per-function numbers of local labels (.LBB12_3, .Lfunc_end12) are dropped before comparing.

usage: python tools/asm_diff.py OLD.s NEW.s      (exit status 1 if a common kernel differs)
"""
import re
import subprocess
import sys


def kernels(path):
    """{mangled kernel name: normalised text}"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, name, body = {}, None, []
    for l in lines:
        l = re.sub(r"(\.L[A-Za-z_]+?)\d+", r"\1", l.split(";")[0]).strip()
        if name is None:
            if l.endswith(":") and l[:-1] in names:
                name, body = l[:-1], []
        elif l == ".Lfunc_end:":
            out[name], name = "\n".join(body), None
        elif l:
            body.append(l)
    assert set(out) == names, "kernel without a body: %s" % sorted(names ^ set(out))
    return out


def demangle(names):
    names = sorted(names)
    if not names:
        return []
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                          check=True).stdout.split("\n")[:len(names)]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    common = set(old) & set(new)
    differ = {k for k in common if old[k] != new[k]}
    for title, group in (("different", differ), ("only in old", set(old) - common),
                         ("only in new", set(new) - common)):
        for n in demangle(group):
            print("%s: %s" % (title, n))
    print("%d kernels in old, %d in new, %d identical, %d different, %d missing, %d new"
          % (len(old), len(new), len(common) - len(differ), len(differ), len(old) - len(common),
             len(new) - len(common)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
