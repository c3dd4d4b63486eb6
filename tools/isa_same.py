#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?  Compares two gfx950
assembly files (hipcc --cuda-device-only -S of kernels.hip, same flags as the
Makefile's) function by function: local labels, comments and directives that
only number things are dropped, everything else must be equal.  Prints the
counts, the functions present on one side only and the ones that differ.
Exit status 1 if a function of OLD is missing from NEW or differs.
usage: isa_same.py OLD.s NEW.s"""
import re
import sys


def funcs(path):
    src = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", src, re.M | re.S):
        body = re.sub(r";.*$", "", m.group(2), flags=re.M)              # comments (they carry block numbers)
        body = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", "L", body)             # local labels are numbered per file
        body = re.sub(r"^\s*\.(loc|file|cfi\w*)\b.*$", "", body, flags=re.M)
        out[m.group(1)] = "\n".join(ln.strip() for ln in body.split("\n") if ln.strip())
    return out


def main():
    old, new = funcs(sys.argv[1]), funcs(sys.argv[2])
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"old {len(old)} functions, new {len(new)}: identical {len(same)}, different {len(differ)}, "
          f"only in old {len(gone)}, only in new {len(added)}")
    for name, ks in (("different", differ), ("only in old", gone), ("only in new", added)):
        for k in ks:
            print(f"  {name}: {k}")
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
