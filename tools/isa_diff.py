#!/usr/bin/env python3
"""isa_diff.py A B -- are two builds' gfx950 kernels the same machine code?

A and B are directories of assembly, one .s per source file, made with the Makefile's flags plus
`--cuda-device-only -S`.  For every function symbol of namespace scde the text from its label to
its .Lfunc_end and its .amdhsa_kernel block (registers, LDS, scratch, occupancy) are compared,
with .LBB<n>_ labels renumbered and comments and .loc / .file / .cfi lines dropped.  Data symbols
are ignored; a kernel that one side holds in more files than the other differs.  Prints one line
per symbol that is not `same` (every symbol with -v) and a summary; exits 1 unless all are same.
"""
import collections
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI|CPI)\d+")
SKIP = re.compile(r"\s*\.(loc|file|cfi_\w+)\b")


def clean(lines):
    out = []
    for ln in lines:
        ln = LABEL.sub(lambda m: ".L" + m.group(1), ln.split(";")[0]).rstrip()
        if ln and not SKIP.match(ln):
            out.append(ln)
    return "\n".join(out)


def functions(directory):
    """symbol -> sorted list of (body, kernel descriptor), one entry per file that defines it"""
    found = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        funcs = {m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(_ZN4scde\w+),@function", ln)] if m}
        body, desc, sets, cur, start = {}, {}, collections.defaultdict(list), None, 0
        for i, ln in enumerate(lines):
            m = re.match(r"(\w+):", ln)
            if cur is None and m and m.group(1) in funcs:
                cur, start = m.group(1), i
            elif cur is not None and ln.startswith(".Lfunc_end"):
                body[cur], cur = clean(lines[start:i]), None
            m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", ln)
            if m and m.group(1) in funcs:
                end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
                desc[m.group(1)] = clean(lines[i:end])
            m = re.match(r"\s*\.set\s+(\w+)\.\w+,", ln)  # the resource counts the descriptor's expressions name
            if m and m.group(1) in funcs:
                sets[m.group(1)].append(ln)
        for sym, text in body.items():
            found[sym].append((text, desc[sym] + "\n" + clean(sets[sym]) if sym in desc else ""))
    return {s: sorted(v) for s, v in found.items()}


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv[1:] if a != "-v"]
    if len(dirs) != 2:
        sys.exit(__doc__)
    a, b = functions(dirs[0]), functions(dirs[1])
    tally = collections.Counter()
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            state = "only in A" if sym in a else "only in B"
        elif a[sym][0][1]:  # a kernel: the same copies on both sides (one each)
            state = "same" if a[sym] == b[sym] else "differs"
        else:  # an out-of-line device function of a header: every file that includes it holds a copy
            state = "same" if set(a[sym]) == set(b[sym]) else "differs"
        tally[state] += 1
        if verbose or state != "same":
            print(f"{state:10s} {sym}")
    kernels = sum(1 for v in a.values() if v[0][1])
    print(f"{sum(tally.values())} symbols ({kernels} kernels in A): " +
          ", ".join(f"{tally[s]} {s}" for s in ("same", "differs", "only in A", "only in B")))
    return 0 if tally["same"] == sum(tally.values()) and tally["same"] > 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
