#!/usr/bin/env python3
"""Function-by-function comparison of the device ISA listings of two builds (volxel_amd/csrc/<unit>.s):
  python tools/isa_compare.py OLD.s NEW.s [NEW.s ...]
The functions of NEW are looked up in the union of its listings; one found in two of them is reported as "DUPLICATE".
A function is "identical" when its instructions match after the block labels are renumbered, "args moved" when they match except
that literals grow by --arg-shift bytes (the kernel-argument offsets behind a grown by-value struct such as VxParams), and
"DIFFERENT" otherwise.  Exit status 1 when a function of OLD is missing from NEW or differs, or NEW holds a duplicate."""
import argparse
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end") or re.match(r"\s*\.size\s", line):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith("."):
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def moved(a, b, shift):
    ta, tb = re.split(r"(0x[0-9a-f]+|\d+)", a), re.split(r"(0x[0-9a-f]+|\d+)", b)
    if len(ta) != len(tb):
        return False
    for u, w in zip(ta, tb):
        if u != w:
            try:
                if int(w, 0) - int(u, 0) != shift:
                    return False
            except ValueError:
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new", nargs="+")
    ap.add_argument("--arg-shift", type=int, default=8)
    a = ap.parse_args()
    old, new = functions(a.old), {}
    bad = 0
    for path in a.new:
        for k, v in functions(path).items():
            if k in new:
                print("DUPLICATE", k, path)
                bad += 1
            new[k] = v
    for k in sorted(old):
        if k not in new:
            print("MISSING  ", k)
            bad += 1
        elif old[k] == new[k]:
            print("identical", k)
        elif len(old[k]) == len(new[k]) and all(x == y or moved(x, y, a.arg_shift) for x, y in zip(old[k], new[k])):
            print("args moved", k, sum(x != y for x, y in zip(old[k], new[k])), "instructions")
        else:
            print("DIFFERENT", k)
            bad += 1
    for k in sorted(set(new) - set(old)):
        print("new      ", k)
    print(f"{len(old)} functions of OLD: {bad} missing, different or duplicate", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
