#!/usr/bin/env python3
"""Lists, for every decode_wave_kernel instance in the compiler's assembly, the vector-memory
instructions and the `s_waitcnt vmcnt(N)` waits in program order (make -C topazdb_amd/csrc asm
writes build/tpz_decode.s).

    python3 tools/vm_waits.py [topazdb_amd/csrc/build/tpz_decode.s] [--kernel decode_wave_kernel]

One line per wait or run of equal VMEM instructions: the line number within the kernel, the
basic block label it sits in, and the instruction. `vmcnt` counts loads and stores in issue
order, so a wait of N placed after the next block's prefetch loads (the run of five
buffer_load_dwordx4) stalls on them unless at least N + 1 younger operations were issued.
The listing is what profiles/prefetch/vm_waits_*.txt hold; reading the control flow between
the lines is left to the reader (the branch targets are printed with the labels).
"""
from __future__ import annotations

import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMEM = re.compile(r"^\s+((?:buffer|global|flat|scratch)_(?:load|store|atomic)\w*)")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*vmcnt\(\d+\).*)$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
LOOP = re.compile(r"Loop Header|Child Loop|Parent Loop")


def kernels(lines, name):
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            m = re.match(r"^(_ZN\S*%s\S*):" % re.escape(name), ln)
            if m:
                start, sym = i, m.group(1)
        elif ln.startswith("\t.size\t" + sym) or ln.startswith(".Lfunc_end"):
            yield sym, lines[start:i]
            start = None


def listing(body):
    out, label, run, run_at, run_n = [], "entry", None, 0, 0

    def flush():
        nonlocal run, run_n
        if run is not None:
            out.append("%6d  %-12s %s%s" % (run_at, label_at, run, " x%d" % run_n if run_n > 1 else ""))
        run, run_n = None, 0

    label_at = label
    for i, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            flush()
            label = m.group(1)
            note = " ; " + ln.split(";", 1)[1].strip() if ";" in ln else ""
            if LOOP.search(ln):
                out.append("%6d  %-12s%s" % (i, label + ":", note))
            continue
        w = WAIT.match(ln)
        if w:
            flush()
            out.append("%6d  %-12s s_waitcnt %s" % (i, label, w.group(1).strip()))
            continue
        v = VMEM.match(ln)
        if v:
            op = v.group(1)
            if op == run and label == label_at:
                run_n += 1
            else:
                flush()
                run, run_at, run_n, label_at = op, i, 1, label
    flush()
    return fold(out)


def fold(rows):
    """Folds a repeated (instruction, wait) pair of one basic block, such as fix_tail's sixteen
    byte loads with a wait each, into one line."""
    key = lambda r: r.split(None, 1)[1]
    out, i = [], 0
    while i < len(rows):
        n = 1
        while (i + 2 * n + 1 < len(rows) and key(rows[i + 2 * n]) == key(rows[i])
               and key(rows[i + 2 * n + 1]) == key(rows[i + 1]) and "s_waitcnt" in rows[i + 1]
               and "s_waitcnt" not in rows[i] and not rows[i].rstrip().endswith(":")):
            n += 1
        if n > 1:
            out.append(rows[i] + "  + " + key(rows[i + 1]).split(None, 1)[1] + "  (pair x%d)" % n)
            i += 2 * n
        else:
            out.append(rows[i])
            i += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm", nargs="?", default=os.path.join(ROOT, "topazdb_amd", "csrc", "build",
                                                           "tpz_decode.s"))
    ap.add_argument("--kernel", default="decode_wave_kernel")
    ap.add_argument("--waits-only", action="store_true")
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    found = False
    for sym, body in kernels(lines, a.kernel):
        found = True
        rows = listing(body)
        waits = [r for r in rows if "s_waitcnt" in r]
        print("== %s: %d lines, %d vmcnt waits" % (sym, len(body), len(waits)))
        for r in (waits if a.waits_only else rows):
            print(r)
        print()
    if not found:
        sys.exit("no kernel matching %r in %s" % (a.kernel, a.asm))


if __name__ == "__main__":
    main()
