"""Kernel-by-kernel comparison of two assembly files of the same unit (hipcc --cuda-device-only -S with the Makefile's flags; the line
is FLAGS in scripts/spill_report.py): one line per kernel, `identical` or `differs`, for a change that must leave some kernels alone.
A kernel's text runs from its label to its .Lfunc_end; only the numbering of local labels and comment lines are ignored.
usage: kernel_isa_diff.py before.s after.s [substring ...]      (substrings: only kernels whose mangled name holds one of them)"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.rstrip("\n")
        if name is None:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.strip()
        if not s or s.startswith(";"):
            continue
        body.append(s)
    return out


def normalised(body):
    seen = {}
    return [re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), s) for s in body]


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    subs = sys.argv[3:]
    for name in sorted(set(a) | set(b)):
        if subs and not any(s in name for s in subs):
            continue
        if name not in a or name not in b:
            print("%-9s %s" % ("only in " + ("before" if name in a else "after"), name))
            continue
        x, y = normalised(a[name]), normalised(b[name])
        print("%-9s %6d -> %6d lines  %s" % ("identical" if x == y else "differs", len(x), len(y), name))
