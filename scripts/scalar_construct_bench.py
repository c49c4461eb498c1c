"""Wall time of sf_construct_scalar (the whole call: host order / uploads, k_scalar_construct, the committed evaluate_all), beside the CPU
oracle's construct_first_fit for ONE replica and the host fixture datasets.construct_graph.  No speed bar: the phase is sequential per
replica by definition; what is recorded is the per-placement latency and how it scales with the replicas resident at once.
Each case: one warm-up + 5 timed launches, a fresh context per launch (the phase needs an unconstructed model), median [min .. max].
usage: scalar_construct_bench.py [out.txt] [case substring ...]      default out: profiles/scalar_construct_bench.txt
       SF_BENCH_DENSE_ORACLE=1 adds the oracle with the reference's dense predicate join at 10k vertices (about a minute of CPU)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import solverforge_amd as sfa
from oracle import sfo
from solverforge_amd import datasets
from solverforge_amd.director import ConstructionHeuristic as H

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scalar_construct_bench.txt")
only = sys.argv[2:]
lines = ["# scripts/scalar_construct_bench.py: sf_construct_scalar, wall time of the call in ms, median [min .. max] of 5 launches after one warm-up,",
         "# a fresh context per launch; us/placement = median / steps of one replica (every replica runs the same placements)"]


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(build, heuristic, launches=6):
    ts, steps = [], 0
    for _ in range(launches):
        d = build()
        d.calculate_score()
        t0 = time.perf_counter()
        d.construct_scalar(0, 0, heuristic=heuristic)
        ts.append((time.perf_counter() - t0) * 1e3)
        steps = d.stats(0)["step_count"]
        ok = bool((d.fresh_score() == d.calculate_score()).all())
        d.close()
        assert ok
    ts = ts[1:]
    return statistics.median(ts), min(ts), max(ts), steps


def cpu_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def graph_case(n, e):
    name = f"graph colouring {n} vertices / {e} edges / 16 colours, FirstFit"
    if only and not any(s in name for s in only):
        return
    g = datasets.make_graph(n, e, 16, seed=0)
    o = sfo.Model.graph_coloring(16, g["adj_off"], g["adj"], g["colors"], indexed=True)
    emit(f"{name}: oracle construct_first_fit (indexed join, 1 replica) {cpu_ms(o.construct_first_fit):.1f} ms; "
         f"datasets.construct_graph {cpu_ms(lambda: datasets.construct_graph(g)):.1f} ms")
    if n <= 10000 and os.environ.get("SF_BENCH_DENSE_ORACLE"):
        o = sfo.Model.graph_coloring(16, g["adj_off"], g["adj"], g["colors"])
        emit(f"{name}: oracle construct_first_fit (the reference's dense join, 1 replica) {cpu_ms(o.construct_first_fit):.1f} ms")
    for R in (1, 256, 3072):
        med, lo, hi, steps = timed(lambda: sfa.build_graph_coloring(g, n_replicas=R), H.FIRST_FIT)
        emit(f"{name}: replicas {R}: {med:.2f} [{lo:.2f} .. {hi:.2f}] ms, {steps} placements, {med * 1e3 / steps:.2f} us/placement, "
             f"{R * steps / med / 1e3:.2f} M placements/s over the replicas")


def jobshop_case():
    name = "mixed job shop 10000 operations x 20 machines (scalar class), CheapestInsertion"
    if only and not any(s in name for s in only):
        return
    p = datasets.make_jobshop(500, 20)
    o = sfo.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], indexed=True)
    emit(f"{name}: oracle construct_first_fit (FirstFit, indexed join, 1 replica) {cpu_ms(o.construct_first_fit):.1f} ms")
    for R in (1, 256, 3072):
        med, lo, hi, steps = timed(lambda: sfa.build_jobshop(p, n_replicas=R), H.CHEAPEST_INSERTION)
        emit(f"{name}: replicas {R}: {med:.2f} [{lo:.2f} .. {hi:.2f}] ms, {steps} placements, {med * 1e3 / steps:.2f} us/placement, "
             f"{R * steps / med / 1e3:.2f} M placements/s over the replicas")


graph_case(10000, 100000)
graph_case(100000, 1000000)
jobshop_case()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
