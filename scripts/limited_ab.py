"""Rate of one list policy with and without a binding limit around the root union, both on the generic engine's traced kernel
(a limit that never binds routes the launch there too).  CVRP-1000, six list leaves, LateAcceptance(400) + BestScore so that a step pulls
its whole cursor: `none` = a root limit no step reaches, `root 4096` / `root 256` = a step ends after that many pulls.  Legs alternate,
rounds in one process; informational -- no bar.
usage: limited_ab.py [replicas] [steps per launch] [rounds]      -> one JSON line per leg and round, then the medians"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solverforge_amd as sfa
from solverforge_amd import datasets

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
LEAVES = ("list_change", "list_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt")
LEGS = (("none", 10 ** 9), ("root 4096", 4096), ("root 256", 256))


def director(limit):
    p = datasets.make_cvrp(1000, 100, 55, seed=0)
    d = sfa.build_cvrp(p, n_replicas=R, leaves=LEAVES)
    d.limit_union(limit)
    d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.LATE_ACCEPTANCE, late_acceptance_size=400, forager=sfa.Forager.BEST_SCORE, random_seed=0))
    d.calculate_score()
    d.phase_start()
    d.solve_steps(1)  # warm-up: allocations of the first launch
    return d


ds = {name: director(limit) for name, limit in LEGS}
rates = {name: [] for name, _ in LEGS}
for rnd in range(ROUNDS):
    for name, _ in LEGS:
        d = ds[name]
        before = d.total_stats()["moves_evaluated"]
        t0 = time.perf_counter()
        d.solve_steps(STEPS)
        dt = time.perf_counter() - t0
        moved = d.total_stats()["moves_evaluated"] - before
        rates[name].append(moved / dt)
        print(json.dumps({"leg": name, "round": rnd, "replicas": R, "steps": STEPS, "wall_s": dt, "moves_evaluated": moved, "moves_per_step": moved / (R * STEPS),
                          "moves_evaluated_per_s": moved / dt}), flush=True)
print(json.dumps({"median_moves_evaluated_per_s": {name: statistics.median(v) for name, v in rates.items()}}), flush=True)
for d in ds.values():
    d.close()
