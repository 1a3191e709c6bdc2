#!/usr/bin/env python3
"""tools/asm_diff.py <dir A> <dir B> — compares two directories of gfx950 assembly (tools/asm_funcs.sh) function by function,
instruction for instruction: comments, directives and the numbering of local labels are left out, everything else must match.
Prints the functions that differ, those only one side has, and the counts."""
import os
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    a_dir, b_dir = sys.argv[1:3]
    same = differ = 0
    only = []
    for f in sorted(os.listdir(a_dir)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(b_dir, f)):
            continue
        fa, fb = functions(os.path.join(a_dir, f)), functions(os.path.join(b_dir, f))
        for name in sorted(set(fa) | set(fb)):
            if name not in fa or name not in fb:
                only.append((f, name, "A" if name in fa else "B"))
            elif fa[name] == fb[name]:
                same += 1
            else:
                differ += 1
                print(f"DIFFERS {f} {name}: {len(fa[name])} -> {len(fb[name])} instructions")
    for f, name, side in only:
        print(f"ONLY IN {side} {f} {name}")
    print(f"{same} functions identical, {differ} differ, {len(only)} on one side only")


if __name__ == "__main__":
    main()
