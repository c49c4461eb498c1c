"""GPU moves/s of one engine on a benchmark workload, without the CPU oracle legs of graph_bench.py / jobshop_bench.py (whose dense oracle
takes over a minute per run): for A/B runs of two library builds, where only the device rate is compared.  Run from the tree under test.
usage: engine_rate.py graph_la|graph_sa|jobshop [timed launches]      -> one JSON line
  graph_la / graph_sa   graph_bench.py's workload and policies (colouring 10k / 100k / 16, 3072 replicas, 100 steps per launch; scalar engine)
  jobshop               jobshop_bench.py's workload (mixed job shop 500 x 20, Bendable<2,1>, 1024 replicas, 100 steps per launch; generic engine)"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import solverforge_amd as sfa
from solverforge_amd import datasets

leg = sys.argv[1]
K = int(sys.argv[2]) if len(sys.argv) > 2 else {"graph_la": 20, "graph_sa": 300, "jobshop": 10}[leg]
ls = 100
if leg == "jobshop":
    d = sfa.build_jobshop(datasets.construct_jobshop(datasets.make_jobshop(500, 20)), n_replicas=1024, makespan=False)
    d.configure(sfa.SolverConfig(random_seed=0))
else:
    d = sfa.build_graph_coloring(datasets.construct_graph(datasets.make_graph(10000, 100000, 16, seed=0)), n_replicas=3072)
    if leg == "graph_sa":
        d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.SIMULATED_ANNEALING, accepted_count_limit=1, random_seed=0))
    else:
        d.configure(sfa.SolverConfig(random_seed=0))
d.calculate_score()
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
print(json.dumps({"leg": leg, "gpu_moves_per_s": (a["moves_evaluated"] - b["moves_evaluated"]) / dt, "seconds": dt, "kernel_ms_per_launch": ms / n,
                  "steps": a["step_count"] - b["step_count"], "score_replica0": d.calculate_score()[0].tolist()}))
