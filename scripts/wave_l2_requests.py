"""The L1 -> L2 request stream of the wave engine's headline kernel, per consumed candidate.

rocprofv3 --pmc passes of `bench.py --replicas 6144 --steps 4 --warmup 3 --pmc-child` (bench.py's own child mode: warm-up and timed launches
only; one residency, because the counter tool crashes above it -- profiles/r04f_pmc_crash_notes.txt).  Every pass holds counters only, nothing
is traced beside them; every pass runs under its own `timeout -k 10`; a pass that fails ends the script -- there is no retry.  Counters are
filtered to k_list_search_wave and averaged over the timed launches.

The rate per second needs the kernel's speed on its real launch shape, which a counter pass does not have: --rate gives it in G moves/s (a
`bench.py` result line's value / 1e9); without it the script runs bench.py once with default arguments, unprofiled, and takes its value.

usage: wave_l2_requests.py [--rate G] [--out FILE] [--timeout S]        (environment such as SF_AMD_WAVE_SPEC_EXTRAS / SF_AMD_LIB is passed on)
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_list_search_wave"
WARMUP, TIMED, REPLICAS = 3, 4, 6144
PASSES = [
    ["TCC_REQ_sum", "TCC_HIT_sum", "TCC_MISS_sum"],
    ["TCP_TCC_READ_REQ_sum", "TCP_TOTAL_CACHE_ACCESSES_sum"],
    ["SQ_INSTS_VMEM_RD", "SQ_BUSY_CYCLES"],
    ["TA_TA_BUSY_sum", "TA_ADDR_STALLED_BY_TC_CYCLES_sum"],
]
SES = 32  # SQ_BUSY_CYCLES is summed over the shader engines
CUS = 256
# MI355X, per CU: what row gathers served from the XCD's L2 reach, and the L2's aggregate rate spread over the CUs
GATHER_GBS_PER_CU = (66.0, 73.0)
L2_AGGREGATE_GBS_PER_CU = 34.5e3 / CUS
REQUEST_BYTES = 64.0


def one_pass(exe, counters, base, i, timeout_s):
    d, work = os.path.join(base, f"pass_{i}"), os.path.join(base, f"work_{i}.json")
    cmd = ["timeout", "-k", "10", str(timeout_s), exe, "--pmc"] + counters + ["--kernel-include-regex", KERNEL, "-f", "csv", "-d", d, "-o", "b", "--",
                                                                              sys.executable, os.path.join(ROOT, "bench.py"), "--replicas", str(REPLICAS), "--steps", str(TIMED),
                                                                              "--warmup", str(WARMUP), "--pmc-child", "--pmc-child-out", work]
    pr = subprocess.run(cmd, cwd=base, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if pr.returncode != 0:
        sys.exit(f"pass {i} ({' '.join(counters)}): exit status {pr.returncode}\n{pr.stderr.decode(errors='replace')[-600:]}")
    per, name = {}, None
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if KERNEL in row["Kernel_Name"]:
                name = row["Kernel_Name"]
                per.setdefault(row["Counter_Name"], []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
    out = {}
    for c in counters:
        v = [x for _, x in sorted(per.get(c, []))][WARMUP:WARMUP + TIMED]
        if len(v) != TIMED:
            sys.exit(f"pass {i}: {len(per.get(c, []))} dispatches of {KERNEL} carry {c}, expected {WARMUP + TIMED}")
        out[c] = sum(v) / TIMED
    return out, json.load(open(work)), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=None, help="G moves/s of bench.py with default arguments")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=90)
    args = ap.parse_args()
    exe = shutil.which("rocprofv3")
    if not exe:
        sys.exit("rocprofv3 not on PATH")
    rate = args.rate
    if rate is None:
        pr = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py")], stdout=subprocess.PIPE, check=True)
        rate = json.loads(pr.stdout.decode().strip().splitlines()[-1])["value"] / 1e9
    base = tempfile.mkdtemp(prefix="sfl2_")
    c, work, kernel = {}, None, None
    try:
        for i, grp in enumerate(PASSES):
            got, w, kernel = one_pass(exe, grp, base, i, args.timeout)
            c.update(got)
            if work is not None and any(w[k] != work[k] for k in ("moves_evaluated", "candidates_scored", "sources_scanned")):
                sys.exit(f"pass {i} did other work than pass 0: {w} / {work}")
            work = w
    finally:
        shutil.rmtree(base, ignore_errors=True)
    cand = work["moves_evaluated"] / work["launches"]  # consumed candidates per launch
    req, vmem = c["TCC_REQ_sum"], c["SQ_INSTS_VMEM_RD"]
    per_cu_s = req / cand * rate * 1e9 / CUS
    gbs = per_cu_s * REQUEST_BYTES / 1e9
    lines = [
        f"kernel                      {kernel}",
        f"extras                      SF_AMD_WAVE_SPEC_EXTRAS={os.environ.get('SF_AMD_WAVE_SPEC_EXTRAS', '(unset: the default)')}",
        f"launch shape of the passes  {work['replicas']} replicas, {work['ls_steps'] // work['launches'] // work['replicas']} steps per launch, mean of {TIMED} launches after {WARMUP}",
        f"consumed candidates/launch  {cand:.0f}   (candidates_scored {work['candidates_scored'] / work['launches']:.0f}, sources_scanned {work['sources_scanned'] / work['launches']:.0f})",
        "counters per launch         " + "  ".join(f"{k}={c[k]:.4g}" for k in sorted(c)),
        f"rate                        {rate:.3f} G moves/s (bench.py, default arguments)",
        "",
        f"vector-memory read wave-instructions per candidate   {vmem / cand:.4f}   ({vmem / cand * 64:.2f} per 64-lane batch)",
        f"L2 requests per candidate (TCC_REQ)                  {req / cand:.4f}   ({req / cand * 64:.1f} per 64-lane batch)",
        f"L2 read requests from the L1s per candidate          {c['TCP_TCC_READ_REQ_sum'] / cand:.4f}   (TCP_TCC_READ_REQ)",
        f"L1 accesses per candidate                            {c['TCP_TOTAL_CACHE_ACCESSES_sum'] / cand:.4f}   (TCP_TOTAL_CACHE_ACCESSES; L1 hit share {1 - c['TCP_TCC_READ_REQ_sum'] / max(c['TCP_TOTAL_CACHE_ACCESSES_sum'], 1):.3f})",
        f"L2 requests per SQ_INSTS_VMEM_RD wave-instruction    {req / vmem:.2f}",
        f"L2 hit share                                         {c['TCC_HIT_sum'] / max(c['TCC_HIT_sum'] + c['TCC_MISS_sum'], 1):.4f}",
        f"L2 requests per second per CU                        {per_cu_s / 1e9:.3f} G/s = {gbs:.1f} GB/s in {REQUEST_BYTES:.0f}-B requests",
        f"  against row gathers from the XCD's L2              {gbs / GATHER_GBS_PER_CU[1]:.2f} - {gbs / GATHER_GBS_PER_CU[0]:.2f} of {GATHER_GBS_PER_CU[0]:.0f} - {GATHER_GBS_PER_CU[1]:.0f} GB/s per CU",
        f"  against the L2's aggregate rate                    {gbs / L2_AGGREGATE_GBS_PER_CU:.2f} of {L2_AGGREGATE_GBS_PER_CU:.0f} GB/s per CU",
        f"address unit: busy share of the kernel's cycles      {c['TA_TA_BUSY_sum'] / max(c['SQ_BUSY_CYCLES'] / SES * CUS, 1):.3f}   stalled by the cache {c['TA_ADDR_STALLED_BY_TC_CYCLES_sum'] / max(c['TA_TA_BUSY_sum'], 1):.3f} of busy",
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
