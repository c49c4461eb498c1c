"""Moves/s under GreatDeluge(0.001) and StepCountingHillClimbing(100) beside LateAcceptance(400), AcceptedCount(256) forager, same
session: graph colouring 10k / 100k / 16 (fused scalar engine) and CVRP-1000 with the six-leaf list policy (generic engine).
Informational: the three acceptors walk different trajectories, so the rates compare policies, not kernels.
A run is as long as its policy makes it: StepCountingHillClimbing accepts only strictly better candidates once `limit` steps have passed
without an improvement, and from a state with none (the constructed colouring starts at [0, 0]) every later step enumerates the whole union
neighbourhood -- 160,000 changes and ~5 x 10^7 swaps per replica.  Name the acceptors to run (la, gd, sc) and give each run a time limit.
`graph_empty` is the same colouring from the all-unassigned start, where improvements abound and StepCounting has a rate to show.
TabuSearch (tabu = move-only 10, the default; tabu4 = entity 7 / value 3 / move 10 / undo 10) runs where its signatures are built: the
colouring (fused scalar engine) and `cvrp2`, CVRP-1000 with the two nearby leaves (wave engine, general replay).  GreatDeluge on the same
workloads runs the same traced kernels, so gd against tabu is the like-for-like cost of the signature and memory work.
usage: acceptor_bench.py [graph|graph_empty|cvrp6|cvrp2|both] [steps per launch] [timed launches] [la,gd,sc,tabu,tabu4]      -> one JSON line per (workload, acceptor)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solverforge_amd as sfa
from solverforge_amd import datasets

which = sys.argv[1] if len(sys.argv) > 1 else "both"
ls = int(sys.argv[2]) if len(sys.argv) > 2 else 100
K = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SIX = ("nearby_change", "nearby_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt")
only = sys.argv[4].split(",") if len(sys.argv) > 4 else ["la", "gd", "sc"]
TABU = getattr(sfa.Acceptor, "TABU_SEARCH", None)  # (absent at commits before TabuSearch: the other acceptors still run there)
TABU_POLICY = {"TabuSearch(move 10)": {}, "TabuSearch(entity 7, value 3, move 10, undo 10)": dict(entity_tabu_size=7, value_tabu_size=3, move_tabu_size=10, undo_move_tabu_size=10)}
ACCEPTORS = [(name, kind) for key, name, kind in (("la", "LateAcceptance(400)", sfa.Acceptor.LATE_ACCEPTANCE), ("gd", "GreatDeluge(0.001)", sfa.Acceptor.GREAT_DELUGE),
                                                   ("sc", "StepCountingHillClimbing(100)", sfa.Acceptor.STEP_COUNTING_HILL_CLIMBING),
                                                   ("tabu", "TabuSearch(move 10)", TABU), ("tabu4", "TabuSearch(entity 7, value 3, move 10, undo 10)", TABU)) if key in only]


def director(workload):
    if workload in ("graph", "graph_empty"):
        g = datasets.make_graph(10000, 100000, 16, seed=0)
        if workload == "graph":
            g = datasets.construct_graph(g)
        return sfa.build_graph_coloring(g, n_replicas=3072), "graph colouring 10k/100k/16, %s start, scalar engine" % ("constructed" if workload == "graph" else "all-unassigned")
    if workload == "cvrp2":
        return sfa.build_cvrp(datasets.make_cvrp(1000, 100, 55, seed=0), n_replicas=4096), "CVRP-1000 two nearby leaves, wave engine"
    return sfa.build_cvrp(datasets.make_cvrp(1000, 100, 55, seed=0), n_replicas=4096, leaves=SIX), "CVRP-1000 six-leaf policy, generic engine"


for workload in (["graph", "cvrp6"] if which == "both" else [which]):
    for name, acceptor in ACCEPTORS:
        d, label = director(workload)
        if name in TABU_POLICY:  # (before the kind is named: sf_solver_configure takes TabuSearch only once its policy was set)
            d.configure_tabu(**TABU_POLICY[name])
        d.configure(sfa.SolverConfig(acceptor=acceptor, random_seed=0))  # the reference's default parameters of each acceptor
        start = d.calculate_score()[0].tolist()
        d.phase_start()
        d.solve_steps(ls)
        d.profile_solve()
        b = d.total_stats()
        t0 = time.perf_counter()
        for _ in range(K):
            d.solve_steps(ls, sync=False)
        d.sync()
        dt = time.perf_counter() - t0
        ms, n = d.profile_solve()
        a = d.total_stats()
        steps = a["step_count"] - b["step_count"]
        print(json.dumps({"workload": label, "acceptor": name, "replicas": d.n_replicas, "gpu_moves_per_s": (a["moves_evaluated"] - b["moves_evaluated"]) / dt,
                          "gpu_steps_per_s": steps / dt, "moves_per_step": (a["moves_evaluated"] - b["moves_evaluated"]) / max(steps, 1),
                          "applied_per_step": (a["moves_applied"] - b["moves_applied"]) / max(steps, 1), "kernel_ms_per_launch": ms / n,
                          "score_start": start, "score_replica0": d.calculate_score()[0].tolist(), "best_of_replicas": max(tuple(int(v) for v in s) for s in d.best_scores())}),
              flush=True)
        d.close()
