"""Rate of the Variable Neighborhood Descent phase (generic engine) on CVRP-1000 from a constructed start (Clarke-Wright savings, then
route-local 2-opt), neighbourhoods [reverse, swap, change]; beside it HillClimbing + BestScore + SelectionOrder.ORIGINAL over the union of
the same three leaves on the same traced kernel, as the like-for-like pull rate.  Informational: no bar.
A short LateAcceptance search with seeds s + r takes the replicas apart first (a descent in Original order draws nothing: without it
every replica would walk the same path).
usage: vnd_bench.py [replicas] [wall seconds of the descent] [steps per launch]      -> one JSON line per leg"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solverforge_amd as sfa
from solverforge_amd import datasets

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WALL = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
LS = int(sys.argv[3]) if len(sys.argv) > 3 else 4
LEAVES = ("list_reverse", "list_swap", "list_change")


def start():
    p = datasets.make_cvrp(1000, 100, 55, seed=0)
    p = dict(p, routes=[[] for _ in p["routes"]])
    d = sfa.build_cvrp(p, n_replicas=R, leaves=LEAVES)
    d.calculate_score()
    d.construct_list_clarke_wright(0, p["customers"], 1)
    d.construct_list_k_opt(0, 2, 1)
    d.configure(sfa.SolverConfig(random_seed=0))  # LateAcceptance(400) + AcceptedCount(256), seeds s + r
    d.phase_start()
    d.solve_steps(20)
    return d


def run(d, label, launch, finished):
    constructed = d.calculate_score()[0].tolist()
    d.phase_start()
    d.profile_solve()
    t0 = time.perf_counter()
    launches = 0
    while time.perf_counter() - t0 < WALL and not finished():
        launch()
        launches += 1
    dt = time.perf_counter() - t0
    ms, n = d.profile_solve()
    a = d.total_stats()
    per = [d.stats(r)["step_count"] for r in range(R)]
    print(json.dumps({"leg": label, "replicas": R, "steps_per_launch": LS, "launches": launches, "wall_s": dt, "kernel_ms": ms,
                      "moves_evaluated": a["moves_evaluated"], "moves_evaluated_per_s": a["moves_evaluated"] / dt, "moves_per_step": a["moves_evaluated"] / max(a["step_count"], 1),
                      "steps_per_replica_min_max": [min(per), max(per)], "applied": a["moves_applied"], "step_ms_per_replica_step": 1e3 * dt / max(max(per), 1),
                      "finished": bool(finished()), "score_start_replica0": constructed, "score_replica0": d.calculate_score()[0].tolist()}), flush=True)


d = start()
d.configure_vnd()
run(d, "vnd [reverse, swap, change]", lambda: d.solve_steps(LS), lambda: d.vnd_done_count() == R)
done = d.vnd_done_count()
print(json.dumps({"leg": "vnd", "replicas_done": done, "idle_steps_replica0": d.vnd_state(0)["idle_steps"]}), flush=True)
d.close()

d = start()
d.configure_union(0, None)  # Sequential over the three leaves in declaration order: the same pulls, one union cursor per step
d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.HILL_CLIMBING, forager=sfa.Forager.BEST_SCORE, random_ties=False, selection_order=sfa.SelectionOrder.ORIGINAL,
                             random_seed=0))
steps_cap = [0]


def hc_launch():
    d.solve_steps(LS)
    steps_cap[0] += LS


run(d, "hill climbing + best score + original, union of the three", hc_launch, lambda: steps_cap[0] >= 4 * LS)
d.close()
