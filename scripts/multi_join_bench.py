"""Fused-search throughput of one scalar class with 1..4 predicate joins (a timetable: 10k lessons choose one of 40 timeslots; hard teacher,
student-group and room conflicts behind COL_EQ partner indices, a soft `same course, timeslots at most 1 apart` join on the interpreter).
Recorded, not targeted: the trial cost of a join is expected to add up per join.
usage: multi_join_bench.py [replicas] [steps per launch] [launches]   -> one JSON line per join count"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import solverforge_amd as sfa
from solverforge_amd import datasets
from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp as P, SelectorKind

R = int(sys.argv[1]) if len(sys.argv) > 1 else 3072
ls = int(sys.argv[2]) if len(sys.argv) > 2 else 100
K = int(sys.argv[3]) if len(sys.argv) > 3 else 5
n, k = 10000, 40
r = datasets.stream(1, 5 * n)
vals0 = (r[:n] % np.uint64(k)).astype(np.int64)
cols = {50: (r[n:2 * n] % np.uint64(500)).astype(np.int32),       # teacher: 20 lessons each
        51: (r[2 * n:3 * n] % np.uint64(400)).astype(np.int32),   # student group: 25 lessons each
        52: (r[3 * n:4 * n] % np.uint64(300)).astype(np.int32),   # room: 33 lessons each
        53: (r[4 * n:5 * n] % np.uint64(1000)).astype(np.int32)}  # course: 10 lessons each
progs = [([(P.COL_EQ, 0, 50), (P.VALUE_EQ, 1)], 0, 1), ([(P.COL_EQ, 0, 51), (P.VALUE_EQ, 1)], 0, 1),
         ([(P.COL_EQ, 0, 52), (P.VALUE_EQ, 1)], 0, 1), ([(P.COL_EQ, 0, 53), (P.VALUE_ABSDIFF_LE, 1, -1, -1, 1)], 1, 3)]
for joins in (1, 2, 3, 4):
    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=R)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, k, True, vals0)
    for f, c in cols.items():
        d.add_fact_column_i32(f, c)
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    for prog, level, weight in progs[:joins]:
        d.add_pair_join(0, prog, level=level, weight=weight)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    d.configure(sfa.SolverConfig(random_seed=0))
    d.calculate_score()
    d.phase_start()
    d.solve_steps(ls)
    b = d.total_stats()
    t0 = time.perf_counter()
    for _ in range(K):
        d.solve_steps(ls, sync=False)
    d.sync()
    dt = time.perf_counter() - t0
    a = d.total_stats()
    moves = a["moves_evaluated"] - b["moves_evaluated"]
    ok = bool((d.fresh_score() == d.calculate_score()).all())
    print(json.dumps({"workload": "timetable 10k lessons / 40 timeslots", "joins": joins, "replicas": R, "gpu_moves_per_s": moves / dt,
                      "gpu_steps_per_s": (a["step_count"] - b["step_count"]) / dt, "fresh_equals_incremental": ok,
                      "score_replica0": d.calculate_score()[0].tolist()}), flush=True)
