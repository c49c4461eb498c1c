"""GPU parity tests of the wave engine's FAST + SMALL kernels (launch modes 2 - 6) at the shapes where their register-level
paths can go wrong: wave-uniform flags (leaf exhaustion, the single-leaf fill, the empty pull), the source cursor (lists longer than 64
and 256, empty routes), the rank table's chunks (V = 65, 129), ring capacity x quota x history length, partial workgroups and every
sf_stats word, and all five instantiations.

Every case asserts the launch mode first (sf_list_wave_layout), then compares a multi-step fused solve with the CPU oracle bit for bit,
replica by replica: working score, best score, working lists, best lists, step_count / moves_evaluated / moves_accepted.  The oracle
keeps no best snapshot of its own: it is stepped one step at a time and its lists are recorded whenever its best score improves (the
rule of update_best_solution).

SF_AMD_NO_COMPACT and SF_AMD_WAVE_WPE are read once per process, so runs under them happen in a fresh child process each (this file
run as a script: it prints its results as JSON), one at a time."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_WORDS = ("step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations",
              "moves_not_doable", "candidates_scored", "sources_scanned", "reserved")
ORACLE_WORDS = STAT_WORDS[:7]
MODE_ENVS = ("SF_AMD_NO_COMPACT", "SF_AMD_WAVE_WPE", "SF_AMD_NODE_GLOBAL")


_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


# ---- problems (built from a hashable key: the oracle's runs are cached per key) ----------------------------------------------------
def _problem(key):
    from solverforge_amd import datasets

    customers, vehicles, capacity, seed, empty = key
    p = datasets.make_cvrp(customers, vehicles, capacity, seed=seed)
    if empty:  # the first `empty` routes handed to the last one: empty routes at the start
        routes = [list(r) for r in p["routes"]]
        for v in range(empty):
            routes[-1] += routes[v]
            routes[v] = []
        p["routes"] = routes
    return p


def _spec(problem, replicas=2, seed=5, launches=(15, 25), max_nearby=20, limit=256, la=400, budget=0, explicit=0):
    """One fused solve: `launches` = steps per sf_solve_steps launch (budget > 0: max steps per sf_solve_moves launch)."""
    return dict(problem=list(problem), replicas=replicas, seed=seed, launches=list(launches), max_nearby=max_nearby, limit=limit, la=la,
                budget=budget, explicit=explicit)


def _step_seeds(spec):
    n = sum(spec["launches"])
    rng = np.random.default_rng(1234 + spec["explicit"])
    return rng.integers(0, 1 << 63, size=(spec["replicas"], n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------
def _gpu_run(spec):
    import solverforge_amd as sfa

    p = _problem(tuple(spec["problem"]))
    R = spec["replicas"]
    d = sfa.build_cvrp(p, n_replicas=R, max_nearby=spec["max_nearby"])
    d.set_engine(2)
    d.configure(sfa.SolverConfig(late_acceptance_size=spec["la"], accepted_count_limit=spec["limit"], random_seed=spec["seed"]))
    if spec["explicit"]:
        d.set_step_seeds(_step_seeds(spec))
    d.calculate_score()
    d.phase_start()
    for n in spec["launches"]:
        if spec["budget"]:
            d.solve_moves(n, spec["budget"])
        else:
            d.solve_steps(n)
    mode = d.wave_layout()[0]
    score, best = d.calculate_score(), d.best_scores()
    fresh = d.fresh_score()
    out = dict(mode=mode, replicas=[])
    for r in range(R):
        out["replicas"].append(dict(score=[int(x) for x in score[r]], best=[int(x) for x in best[r]], fresh=[int(x) for x in fresh[r]],
                                    lists=d.working_lists(0, r), best_lists=d.working_lists(0, r, best=True), stats=d.stats(r)))
    d.close()
    return out


def _child_run(spec, env):
    e = {k: v for k, v in os.environ.items() if k not in MODE_ENVS}
    e.update(env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(spec)], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


# ---- the oracle's run ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(problem, replica_seed, steps, max_nearby, limit, la, seeds):
    """(score, best score, lists, best lists, stats, most candidates accepted in one step) after `steps` steps of one replica."""
    sfo = _SFO["sfo"]
    p = _problem(problem)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=la, limit=limit, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=max_nearby, random_seed=replica_seed)
    if seeds is not None:
        o.set_step_seeds(np.array(seeds, dtype=np.uint64))
    o.phase_start()
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    accepted, most = 0, 0
    for _ in range(steps):
        o.steps(1)
        a = o.stats()["moves_accepted"]
        most, accepted = max(most, a - accepted), a
        b = o.best_score()
        if (b != best).any():
            best, best_lists = b.copy(), o.get_lists(0)
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists,
                stats=o.stats(), most_accepted=most)


@functools.lru_cache(maxsize=None)
def _oracle_budget_steps(problem, replica_seed, launches, budget, max_nearby, limit, la):
    """Steps one replica runs in budgeted launches, from the oracle alone: a launch ends after the step in which the candidates it
    generated reach `budget` (sf_solve_moves), or after its `launches[i]` steps."""
    sfo = _SFO["sfo"]
    p = _problem(problem)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=la, limit=limit, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=max_nearby, random_seed=replica_seed)
    o.phase_start()
    steps = 0
    for n in launches:
        at_start = o.stats()["moves_generated"]
        for _ in range(n):
            o.steps(1)
            steps += 1
            if o.stats()["moves_generated"] - at_start >= budget:
                break
    return steps


def _check(spec, got, mode, words=("step_count", "moves_evaluated", "moves_accepted")):
    assert got["mode"] == mode, got["mode"]
    seeds = _step_seeds(spec) if spec["explicit"] else None
    wants = []
    for r, g in enumerate(got["replicas"]):
        if spec["budget"]:  # where the budget ends each launch is the oracle's word, not the library's
            steps = _oracle_budget_steps(tuple(spec["problem"]), spec["seed"] + r, tuple(spec["launches"]), spec["budget"], spec["max_nearby"],
                                         spec["limit"], spec["la"])
            assert g["stats"]["step_count"] == steps, (r, g["stats"]["step_count"], steps)
        else:
            steps = sum(spec["launches"])
        w = _oracle_run(tuple(spec["problem"]), spec["seed"] + r, steps, spec["max_nearby"], spec["limit"], spec["la"],
                        None if seeds is None else tuple(int(x) for x in seeds[r]))
        assert g["score"] == w["score"], r
        assert g["fresh"] == w["score"], r
        assert g["best"] == w["best"], r
        assert g["lists"] == w["lists"], r
        assert g["best_lists"] == w["best_lists"], r
        for k in words:
            assert g["stats"][k] == w["stats"][k], (r, k)
        wants.append(w)
    return wants


# ---- 1. flags as scalars: exhaustion, the single-leaf fill, the empty pull; resolve()'s skip-empty loop -------------------------------
def test_leaf_exhaustion_small_model():
    """8 customers on 2 vehicles: a step runs out of candidates before the 256th accepted one (checked on the oracle alone first), so
    both leaves are exhausted in every step -- the `ex` flags, the single-leaf fill and the pull that finds an empty ring."""
    spec = _spec((8, 2, 30, 3, 0), replicas=3, launches=(20, 20))
    for r in range(3):
        w = _oracle_run(tuple(spec["problem"]), spec["seed"] + r, 40, 20, 256, 400, None)
        assert 0 < w["most_accepted"] < 256, w["most_accepted"]
    _check(spec, _gpu_run(spec), 5, ORACLE_WORDS)


def test_empty_routes_at_the_start():
    """12 customers on 6 vehicles, the first two routes empty at the start: resolve() skips them."""
    key = (12, 6, 30, 4, 2)
    assert sum(1 for r in _problem(key)["routes"] if not r) >= 2
    spec = _spec(key, replicas=3, launches=(20, 20))
    _check(spec, _gpu_run(spec), 5, ORACLE_WORDS)


# ---- 2. the source cursor: one list longer than 64 / 256 -------------------------------------------------------------------------------
@pytest.mark.parametrize("customers", [100, 300])
def test_one_long_list(customers):
    """One vehicle: offsets past the 64 a cursor caches (the vbase chunk change) and positions that need more than 8 bits."""
    spec = _spec((customers, 1, 10_000, 21, 0), launches=(12, 13))
    _check(spec, _gpu_run(spec), 5)


# ---- 3. rank-table chunks: V = 65, 129 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("customers,vehicles", [(200, 65), (300, 129)])
def test_rank_table_chunks(customers, vehicles):
    """Two and three 64-route chunks of the per-leaf tables; past 128 routes the step prologue takes its scalar hashes (no coprime masks)."""
    spec = _spec((customers, vehicles, 55, 9, 0), launches=(12, 13))
    _check(spec, _gpu_run(spec), 5)


# ---- 4. ring capacity x quota x history length, two launches ----------------------------------------------------------------------------
@pytest.mark.parametrize("la", [1, 400])
@pytest.mark.parametrize("limit", [1, 4, 256])
@pytest.mark.parametrize("max_nearby", [1, 20, 64])
def test_ring_quota_history(max_nearby, limit, la):
    spec = _spec((60, 6, 55, 3, 0), max_nearby=max_nearby, limit=limit, la=la)
    _check(spec, _gpu_run(spec), 5, ORACLE_WORDS)


# ---- 5. partial workgroups and every counter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replicas,budget", [(5, 0), (9, 0), (5, 3000), (9, 3000)])
def test_partial_workgroups_and_counters(replicas, budget):
    """5 and 9 replicas (workgroups of 4 waves); fixed-step launches, and budgeted launches that end the replicas at different step
    counts.  Every sf_stats word per replica: default layout == the wide layout (launch mode 2), and == the oracle where it has the word."""
    spec = _spec((60, 6, 55, 3, 0), replicas=replicas, launches=(500, 500) if budget else (15, 25), budget=budget, limit=16, la=7)
    got = _gpu_run(spec)
    _check(spec, got, 5, ORACLE_WORDS)
    wide = _child_run(spec, {"SF_AMD_NO_COMPACT": "1"})
    _check(spec, wide, 2, ORACLE_WORDS)
    for r in range(replicas):
        for k in STAT_WORDS:
            assert got["replicas"][r]["stats"][k] == wide["replicas"][r]["stats"][k], (r, k)
        assert got["replicas"][r]["stats"]["sources_scanned"] > 0 and got["replicas"][r]["stats"]["candidates_scored"] > 0
    if budget:
        assert len({g["stats"]["step_count"] for g in got["replicas"]}) > 1  # ended on the budget, at different distances


# ---- 6. every FAST + SMALL instantiation --------------------------------------------------------------------------------------------------
MODES = [({"SF_AMD_NO_COMPACT": "1"}, 2), ({"SF_AMD_WAVE_WPE": "4"}, 2), ({"SF_AMD_WAVE_WPE": "5"}, 4), ({}, 5), ({"SF_AMD_NODE_GLOBAL": "1"}, 6)]


def test_every_instantiation():
    """The default row of test_ring_quota_history under launch modes 2, 4, 5, 6, with random and with explicit step seeds: each mode in a
    child of its own, all equal to each other and to the oracle.  (This model is small enough for 16 wide slices per CU, so capped at 4
    waves per SIMD it runs launch mode 2; test_compact_slice_at_four_waves takes mode 3.)"""
    runs = {}
    for explicit in (0, 1):
        spec = _spec((60, 6, 55, 3, 0), explicit=explicit)
        for env, mode in MODES:
            got = _child_run(spec, env)
            _check(spec, got, mode, ORACLE_WORDS)
            runs[(explicit, json.dumps(env))] = got["replicas"]
        first = runs[(explicit, json.dumps(MODES[0][0]))]
        for env, _ in MODES[1:]:
            assert runs[(explicit, json.dumps(env))] == first, env
    assert runs[(0, "{}")] != runs[(1, "{}")]  # the explicit seeds were used


def test_compact_slice_at_four_waves():
    """Launch mode 3: the COMPACT slice compiled for 4 waves per SIMD, taken when the wide slice is too large for 16 replicas per CU
    (1500 customers: 13 wide slices, 16 compact ones).  Compared with the oracle and, every sf_stats word included, with the wide
    layout's run (launch mode 2) of the same solve."""
    for explicit in (0, 1):
        spec = _spec((1500, 100, 55, 4, 0), launches=(6, 6), explicit=explicit)
        got = _child_run(spec, {"SF_AMD_WAVE_WPE": "4"})
        _check(spec, got, 3, ORACLE_WORDS)
        wide = _child_run(spec, {"SF_AMD_NO_COMPACT": "1"})
        _check(spec, wide, 2, ORACLE_WORDS)
        assert got["replicas"] == wide["replicas"]


if __name__ == "__main__":  # the child: one run, its results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps(_gpu_run(json.loads(sys.argv[1]))))
