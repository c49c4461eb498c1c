"""Route-local 2-opt (sf_construct_list_k_opt) with and without the time-window hook: wall time of one call (launch + the committed
score, synchronous) on a fresh context per launch -- the phase changes the lists, so a second call on the same context would time a
no-op.  One warm-up launch, then `--launches` timed ones: median, min, max (the spread the comparison has to be read against).
Legs (comma-separated in --legs):
  mode1      CVRP-1000 / 100, capacity 55, round-robin start, feasible_mode 1, --replicas replicas: the leg that must not move against
             the parent commit (it launches the same instantiation; needs nothing this commit adds, so it runs on a parent checkout too)
  tw         the same size with windows (datasets.make_cvrptw, slack 1000 and 3000): mode 1, mode 2 as the host range check picks it
             (the composed fold) and mode 2 with the checked lane-serial walk forced
  one_route  130 and 1000 customers in ONE route (capacity out of the way, slack 3000, --one-route-replicas replicas): the shape in which
             the hook is evaluated most often; composed vs walk (the walk only up to --walk-max-route visits)
  oracle     the CPU oracle's time for one replica of each case above, for scale only
python scripts/kopt_tw_bench.py [--replicas 24576] [--launches 5] [--legs mode1,tw,one_route,oracle] > profiles/kopt_tw_bench.txt"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BIG = 10**6


def timed(p, replicas, mode, launches, force_walk=None, max_sweeps=1000):
    import solverforge_amd as sfa

    secs, path, stats = [], None, None
    for it in range(launches + 1):
        d = sfa.build_cvrp(p, n_replicas=replicas)
        d.calculate_score()
        if force_walk is not None:
            path = d.time_window_path(0, force_walk=force_walk)
        d.construct_list_k_opt(0, 3, mode, max_sweeps)  # k != 2: scored no-op; allocates the counters outside the timed call
        t0 = time.perf_counter()
        sc = d.construct_list_k_opt(0, 2, mode, max_sweeps)
        t1 = time.perf_counter()
        if it > 0:  # the first launch is the warm-up
            secs.append(t1 - t0)
        st = d.stats(0)
        stats = {"candidates": st["moves_generated"], "accepted": st["moves_accepted"], "score": sc[0].tolist()}
        d.close()
    out = {"replicas": replicas, "feasible_mode": mode, "launches": launches, "median_s": statistics.median(secs), "min_s": min(secs), "max_s": max(secs)}
    if path:
        out["path"] = path
    out.update(stats)
    return out


def oracle_seconds(p, mode, max_sweeps=1000):
    from oracle import sfo

    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    if "time_windows" in p:
        lo, hi = p["time_windows"]
        o.set_time_windows(lo, hi, p["service"], p["travel"], p["departure"])
    t0 = time.perf_counter()
    st = o.construct_list_k_opt(2, mode, max_sweeps)
    return {"oracle_s": time.perf_counter() - t0, "oracle_candidates": int(st[0]), "oracle_accepted": int(st[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=24576, help="replicas of the CVRP-1000 legs (bench.py's M2 leg: 24,576 per GPU)")
    ap.add_argument("--one-route-replicas", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--walk-max-route", type=int, default=200,
                    help="one_route legs: the forced checked walk is timed only up to this route length (at 1000 visits one launch of it runs for minutes)")
    ap.add_argument("--legs", default="mode1,tw,one_route,oracle")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    from solverforge_amd import datasets

    def emit(case, row):
        print(json.dumps(dict({"case": case}, **row)), flush=True)

    if "mode1" in legs:
        p = datasets.make_cvrp(1000, 100, 55, seed=0)
        emit("cvrp-1000/100 cap 55, no windows", timed(p, a.replicas, 1, a.launches))
    cases = []
    if "tw" in legs:
        for slack in (1000, 3000):
            cases.append((f"cvrp-1000/100 cap 55, slack {slack}", datasets.make_cvrptw(1000, 100, 55, seed=0, slack=slack, tw_seed=3), a.replicas, True))
    if "one_route" in legs:
        cases.append(("one route of 130, slack 3000", datasets.make_cvrptw(130, 9, BIG, seed=21, slack=3000, tw_seed=2, one_route=True), a.one_route_replicas, False))
        cases.append(("one route of 1000, slack 3000", datasets.make_cvrptw(1000, 100, BIG, seed=0, slack=3000, tw_seed=3, one_route=True), a.one_route_replicas, False))
    for name, p, replicas, with_mode1 in cases:
        if with_mode1:
            emit(name, timed(p, replicas, 1, a.launches))
        longest = max(len(rt) for rt in p["routes"])
        for force in (False, True):
            if force and not with_mode1 and longest > a.walk_max_route:
                emit(name, {"replicas": replicas, "feasible_mode": 2, "path": "walk", "median_s": None, "note": "not timed: above --walk-max-route"})
                continue
            row = timed(p, replicas, 2, a.launches, force_walk=force)
            if "oracle" in legs and not force:
                row.update(oracle_seconds(p, 2))
            emit(name, row)


if __name__ == "__main__":
    main()
