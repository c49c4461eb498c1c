"""Where the scalar-register spills of a wave-engine kernel sit: static counts per marked region of one kernel in the .s of a wave
unit (spill reloads / stores through the lanes of the spill VGPRs, wait states, instruction mix) -- the tool behind DESIGN 16.

usage: spill_report.py [file.s] kernel-substring [kernel-substring ...]
       spill_report.py --all            the five FAST + SMALL instantiations of the L = 2 unit (launch modes 2, 3, 4, 5, 6)

Without a .s the L = 2 wave unit is compiled with -DSF_ISA_MARK into a temporary directory.  A region x is what control flow reaches
between the marks x_begin and x_end (the compiler moves blocks around, so the regions are followed through the branches, not read off
the text); resolve()'s slow path is inlined several times and is one row.  The kernels with the lockstep round have two more
regions, sym_fill and sym_replay -- the round's fill loop and its batch; the round's copy of the paired pass lies inside sym_fill and counts in
`pair` (and `pair_rest`, `resolve_slow`) as well, so those rows hold two copies there: sym_fill less one copy of `pair` is the round's fill glue.
  spill VGPR   a VGPR that appears only as the destination of v_writelane or the source of v_readlane
  step loop    the backward branch with the largest span
  const/carried  a reload of a slot (register, lane) written only before the step loop / written inside it
  vector-memory waits   per region, the vector-memory loads and the s_waitcnt that name vmcnt, as "n x vmcnt(k)" -- here an instruction counts in
                 its INNERMOST region only, so `pair` is the paired pass without resolve()'s slow path (resolve_slow) and without the gen_rest
                 continuation (pair_rest): its common path.  A load that stays in flight across the pass shows as `pair` with loads and no wait;
                 the one wait for the loads of the pass before is scheduled in front of the pair_begin mark and counts in `fill`.  The last column
                 is the text order of the two (L a load, w a wait), which is not the order of execution.
Opcodes are classified by prefix (scripts/isa_blocks.py: cat)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_blocks import cat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solverforge_amd", "csrc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I/opt/rocm/include -DSF_TU_L=2 -DSF_ISA_MARK --cuda-device-only -S"
# (mode, template arguments after <L, TRACE, MODE>: COMPACT, WPE, NODEG) of the FAST + SMALL instantiations
FAST_SMALL = [(2, "Lb0ELi4ELb0E"), (3, "Lb1ELi4ELb0E"), (4, "Lb1ELi5ELb0E"), (5, "Lb1ELi6ELb0E"), (6, "Lb1ELi4ELb1E")]


def build_s(out_dir):
    path = os.path.join(out_dir, "list_wave_2.s")
    subprocess.check_call(["hipcc"] + FLAGS.split() + ["sf_tu_list_wave.hip", "-o", path], cwd=CSRC)
    return path


def vregs(tok):
    """VGPR numbers an operand names: v7 or v[4:5]."""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return [int(m.group(1))]
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return []


def kernel_lines(lines, needle):
    start = [i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and needle in l.split(":")[0]]
    if not start:
        raise SystemExit("no kernel matches " + needle)
    s = start[0]
    e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
    info = {}
    for l in lines[e : e + 80]:
        m = re.match(r"; (TotalNumSgprs|NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", l)
        if m:
            info.setdefault(m.group(1), int(m.group(2)))
    name = lines[s].split(":")[0]
    for i, l in enumerate(lines):
        if l.strip() == ".name:           " + name or (l.strip().startswith(".name:") and l.split()[-1] == name):
            for l2 in lines[i : i + 8]:
                if "sgpr_spill_count" in l2:
                    info["SgprSpill"] = int(l2.split()[-1])
    return name, lines[s + 1 : e], info


def report(path, needle, out=sys.stdout):
    name, body, info = kernel_lines(open(path).read().split("\n"), needle)
    # basic blocks of (kind, ...) items: ("ins", op, operands, index) | ("mark", name)
    blocks, labels, ins = [[]], {}, []
    for l in body:
        s = l.strip()
        m = re.match(r"; SF_MARK (\S+)", s)
        if m:
            blocks[-1].append(("mark", m.group(1)))
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            if blocks[-1]:
                blocks.append([])
            labels[m.group(1)] = len(blocks) - 1
            continue
        if not s or s.startswith((";", ".")):
            continue
        s = s.split(";")[0].strip()
        op, _, rest = s.partition(" ")
        ops = [t.strip() for t in rest.split(",")] if rest else []
        blocks[-1].append(("ins", op, ops, len(ins)))
        ins.append((op, ops))
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append([])
    first = [next((it[3] for it in b if it[0] == "ins"), None) for b in blocks]
    # spill registers
    lane_use, other_use = set(), set()
    for op, ops in ins:
        if op.startswith("v_writelane"):
            lane_use.update(vregs(ops[0]))
            for t in ops[1:]:
                other_use.update(vregs(t))
        elif op.startswith("v_readlane"):
            lane_use.update(vregs(ops[1]))
        else:
            for t in ops:
                for u in re.findall(r"v\[\d+:\d+\]|v\d+", t):
                    other_use.update(vregs(u))
    spill = lane_use - other_use
    # step loop: the backward branch with the largest span
    lo = hi = 0
    for k, (op, ops) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")) and ops and ops[-1] in labels:
            t = next((f for f in first[labels[ops[-1]] :] if f is not None), len(ins))
            if t <= k and k - t > hi - lo:
                lo, hi = t, k
    written_in, written = set(), set()
    for k, (op, ops) in enumerate(ins):
        if op.startswith("v_writelane") and vregs(ops[0])[0] in spill:
            slot = (vregs(ops[0])[0], ops[2])
            written.add(slot)
            if lo <= k <= hi:
                written_in.add(slot)
    # the regions an instruction lies in: walk the control flow graph from the entry; x_begin opens x, x_end closes it (a block takes the
    # open regions of the first path that reaches it -- the marks are nested the same way on every path)
    region = [None] * len(ins)
    seen = [False] * len(blocks)
    work = [(0, ())]
    while work:
        b, st = work.pop()
        if b >= len(blocks) or seen[b]:
            continue
        seen[b] = True
        succ = [b + 1]
        for it in blocks[b]:
            if it[0] == "mark":
                n = it[1]
                if n.endswith("_begin"):
                    st = st + (n[:-6],)
                elif n.endswith("_end") and n[:-4] in st:
                    k = len(st) - 1 - st[::-1].index(n[:-4])
                    st = st[:k]
                continue
            _, op, ops, k = it
            region[k] = st
            if op.startswith("s_endpgm"):
                succ = []
            elif op.startswith("s_branch"):
                succ = [labels[ops[-1]]] if ops[-1] in labels else []
            elif op.startswith("s_cbranch") and ops[-1] in labels:
                succ = [labels[ops[-1]], b + 1]
        for t in succ:
            work.append((t, st))
    rows = {}
    order = []
    for k, (op, ops) in enumerate(ins):
        st = region[k]
        inl = lo <= k <= hi
        names = ["(not reached)"] if st is None else list(dict.fromkeys(st)) if st else ["(rest of the step loop)" if inl else "(outside the step loop)"]
        if inl:
            names.append("step loop, all")
        for n in names:
            if n not in rows:
                rows[n] = dict(rc=0, rk=0, st=0, nop=0, ws=0, salu=0, valu=0, lds=0, vmem=0, n=0, vmw={}, vml=0, seq="")
                order.append(n)
            row = rows[n]
            row["n"] += 1
            if not st or n == st[-1]:  # the vector-memory columns: innermost region only
                if op == "s_waitcnt":
                    m = re.search(r"vmcnt\((\d+)\)", " ".join(ops))
                    if m:
                        row["vmw"][int(m.group(1))] = row["vmw"].get(int(m.group(1)), 0) + 1
                        row["seq"] += "w"
                elif op.startswith(("global_load", "buffer_load", "flat_load")):
                    row["vml"] += 1
                    row["seq"] += "L"
            if op.startswith("v_readlane") and vregs(ops[1])[0] in spill:
                row["rk" if (vregs(ops[1])[0], ops[2]) in written_in else "rc"] += 1
            elif op.startswith("v_writelane") and vregs(ops[0])[0] in spill:
                row["st"] += 1
            elif op == "s_nop":
                row["nop"] += 1
                row["ws"] += int(ops[0], 0) + 1
            else:
                c = cat(op)
                if c in ("salu", "branch", "smem", "wait"):
                    row["salu"] += 1
                elif c in ("valu", "lane"):
                    row["valu"] += 1
                elif c in ("lds", "vmem"):
                    row[c] += 1
    p = lambda *a: print(*a, file=out)
    p("kernel", name)
    p("  resources: SGPRs %s  VGPRs %s  scratch %s B  occupancy %s  static LDS %s B  SGPR spills %s" % tuple(
        info.get(k, "?") for k in ("TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize", "SgprSpill")))
    p("  spill VGPRs: %s   slots %d (written only before the step loop %d, inside it %d)" % (
        " ".join("v%d" % v for v in sorted(spill)) or "none", len(written), len(written - written_in), len(written_in)))
    p("  %-26s %6s | %7s %8s %8s | %6s %10s | %6s %6s %6s %5s %5s" % ("region (nested ones count in their parent too)", "instr", "reloads", "constant", "carried", "stores",
                                                                    "rl+st", "s_nop", "(wait)", "scalar", "vector", "mem"))
    for n in sorted(order, key=lambda n: (n.startswith("("), n == "step loop, all", n)):
        row = rows[n]
        p("  %-47s %6d | %7d %8d %8d | %6d %10d | %6d %6d %6d %6d %5d" % (n, row["n"], row["rc"] + row["rk"], row["rc"], row["rk"], row["st"], row["rc"] + row["rk"] + row["st"],
                                                                   row["nop"], row["ws"], row["salu"], row["valu"], row["lds"] + row["vmem"]))
    p("  vector-memory loads and waits, each in its innermost region (last column: text order, L a load, w a wait that names vmcnt)")
    for n in sorted(order, key=lambda n: (n.startswith("("), n == "step loop, all", n)):
        row = rows[n]
        if n == "step loop, all" or n.startswith("("):
            continue
        p("  %-47s loads %3d | waits %s | %s" % (n, row["vml"], " ".join("%d x vmcnt(%d)" % (c, k) for k, c in sorted(row["vmw"].items())) or "none", row["seq"]))
    p("")


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if args and args[0].endswith(".s"):
        path, args = args[0], args[1:]
    tmp = None
    if path is None:
        tmp = tempfile.TemporaryDirectory()
        path = build_s(tmp.name)
    if args == ["--all"] or not args:
        for mode, targs in FAST_SMALL:
            print("launch mode", mode)
            report(path, "k_list_search_waveILi2ELb0ELi2E" + targs)
    else:
        for needle in args:
            report(path, needle)
