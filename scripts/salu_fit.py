"""Where the scalar instructions of the wave kernel go: SQ_INSTS_SALU / SQ_INSTS_VALU of bench.py's timed launches at several (max_nearby,
AcceptedCount limit) settings, fitted as  a x steps + b x sources + c x replay batches + d x source entities  (batches = candidates scored / 64).
The entities are DERIVED, not counted: a leaf walks its entities' lists in full, so it enters resolve()'s per-entity path once per list, i.e.
sources / mean list length times (the partial list at a step's end goes to the per-step term).  Two rows at other list counts (50 and 125 lists
for the same 1,000 customers: mean lengths 20 and 8, both inside the V <= 128 gate of the lane-parallel hashes) make the term separable from the
sources.
usage: salu_fit.py <out.json>     (runs rocprofv3 --pmc children of bench.py at 6,144 replicas)"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUSTOMERS = 1000  # passed to bench.py and used for the mean list length of the derived entity count
rows = []
for k, lim, veh in [(20, 256, 100), (5, 256, 100), (40, 256, 100), (20, 64, 100), (20, 1024, 100), (10, 128, 100), (20, 256, 50), (20, 256, 125)]:
    base = tempfile.mkdtemp(prefix="salufit_", dir="/tmp")
    work = os.path.join(base, "work.json")
    cmd = ["rocprofv3", "--pmc", "SQ_INSTS_SALU", "SQ_INSTS_VALU", "--kernel-include-regex", "k_list_search_wave", "-f", "csv", "-d", base, "-o", "b", "--", sys.executable,
           os.path.join(R, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3", "--replicas", "6144", "--ls-steps", "200", "--max-nearby", str(k), "--accepted-limit", str(lim), "--vehicles", str(veh), "--customers", str(CUSTOMERS),
           "--pmc-child", "--pmc-child-out", work]
    try:  # one try: after a counter pass that failed or ran into its time limit nothing further is started on the device
        pr = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    except subprocess.TimeoutExpired:
        sys.exit(f"salu_fit: the pass at max_nearby {k}, limit {lim}, {veh} lists ran into its time limit; stopping")
    if pr.returncode != 0:
        sys.exit(f"salu_fit: the pass at max_nearby {k}, limit {lim}, {veh} lists ended with status {pr.returncode}; stopping")
    per = {}
    for f in glob.glob(os.path.join(base, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            per.setdefault(row["Counter_Name"], []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
    w = json.load(open(work))
    salu = sum(v for _, v in sorted(per["SQ_INSTS_SALU"])[3:]); valu = sum(v for _, v in sorted(per["SQ_INSTS_VALU"])[3:])
    rows.append({"max_nearby": k, "limit": lim, "vehicles": veh, "entities": w["sources_scanned"] * veh / float(CUSTOMERS), "salu": salu, "valu": valu, "steps": w["ls_steps"], "sources": w["sources_scanned"], "batches": w["candidates_scored"] / 64.0,
                 "moves": w["moves_evaluated"]})
    shutil.rmtree(base, ignore_errors=True)
    print(json.dumps(rows[-1]), flush=True)
A = np.array([[r["steps"], r["sources"], r["batches"], r["entities"]] for r in rows], dtype=np.float64)
fit = {}
for name in ("salu", "valu"):
    y = np.array([r[name] for r in rows], dtype=np.float64)
    coef, res, rank, sv = np.linalg.lstsq(A, y, rcond=None)
    pred = A @ coef
    fit[name] = {"per_step": coef[0], "per_source": coef[1], "per_replay_batch": coef[2], "per_entity": coef[3], "max_rel_err": float(np.max(np.abs(pred - y) / y))}
    d = rows[0]
    fit[name]["share_at_default"] = {"steps": coef[0] * d["steps"] / d[name], "sources": coef[1] * d["sources"] / d[name], "batches": coef[2] * d["batches"] / d[name], "entities": coef[3] * d["entities"] / d[name]}
json.dump({"rows": rows, "fit": fit}, open(sys.argv[1], "w"), indent=1)
print(json.dumps(fit, indent=1))
