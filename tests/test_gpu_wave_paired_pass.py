"""GPU parity tests of the paired generation pass of the wave engine's FAST + SMALL kernels (launch modes 2 - 6) at the smallest shapes
at which its register-level paths can go wrong: neighbour rows shorter than, equal to and just longer than a half (32 entries) and a
chunk (64) -- the row entries stay raw in flight and are blanked where the key is taken --, positions saturated in the 16-bit node
table with the per-step flag going both ways, equal-distance groups wider than a half and wider than a chunk (the inversion loop, the
gen_rest continuation, the serial top-k over the rank-only table), max_nearby around the ring sizes, one leaf running dry (the
single-leaf path with its rotated key), and all five instantiations.

The method is that of test_gpu_wave_register_paths.py: every case asserts the launch mode first (sf_list_wave_layout), then compares a
fused multi-launch solve with the CPU oracle bit for bit, replica by replica: working score, best score, fresh score, working lists,
best lists and the seven counters the oracle keeps.  The oracle is stepped one step at a time; its lists are recorded whenever its best
score improves, and the length of the longest list after every step (the saturation cases assert their precondition on it).

SF_AMD_NO_COMPACT, SF_AMD_WAVE_WPE and SF_AMD_NODE_GLOBAL are read once per process, so runs under them happen in a fresh child process
each (this file run as a script: it prints its results as JSON), one at a time."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_WORDS = ("step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations", "moves_not_doable")
MODE_ENVS = ("SF_AMD_NO_COMPACT", "SF_AMD_WAVE_WPE", "SF_AMD_NODE_GLOBAL")
# (environment, launch mode it selects for a model small enough for 24 slices per CU)
MODES = [({"SF_AMD_NO_COMPACT": "1"}, 2), ({"SF_AMD_WAVE_WPE": "4"}, 2), ({"SF_AMD_WAVE_WPE": "5"}, 4), ({}, 5), ({"SF_AMD_NODE_GLOBAL": "1"}, 6)]

_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


# ---- problems (built from a hashable key: the oracle's runs are cached per key) ----------------------------------------------------
def _problem(key):
    from solverforge_amd import datasets

    customers, vehicles, capacity, seed, fold, coord_range = key
    p = datasets.make_cvrp(customers, vehicles, capacity, seed=seed, coord_range=coord_range)
    if fold:  # the first `fold` routes handed to the last one: one long route, empty routes at the start
        routes = [list(r) for r in p["routes"]]
        for v in range(fold):
            routes[-1] += routes[v]
            routes[v] = []
        p["routes"] = routes
    return p


def _key(customers, vehicles, capacity=10_000, seed=3, fold=0, coord_range=1000):
    return (customers, vehicles, capacity, seed, fold, coord_range)


def _spec(problem, replicas=2, seed=5, launches=(15, 25), max_nearby=20, limit=256, la=400):
    return dict(problem=list(problem), replicas=replicas, seed=seed, launches=list(launches), max_nearby=max_nearby, limit=limit, la=la)


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------
def _gpu_run(spec):
    import solverforge_amd as sfa

    p = _problem(tuple(spec["problem"]))
    R = spec["replicas"]
    d = sfa.build_cvrp(p, n_replicas=R, max_nearby=spec["max_nearby"])
    d.set_engine(2)
    d.configure(sfa.SolverConfig(late_acceptance_size=spec["la"], accepted_count_limit=spec["limit"], random_seed=spec["seed"]))
    d.calculate_score()
    d.phase_start()
    for n in spec["launches"]:
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
def _oracle_run(problem, replica_seed, steps, max_nearby, limit, la):
    """Scores, lists and counters after `steps` steps of one replica, and the longest list's length at the start and after every step."""
    sfo = _SFO["sfo"]
    p = _problem(problem)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=la, limit=limit, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=max_nearby, random_seed=replica_seed)
    o.phase_start()
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    longest = [max(len(r) for r in best_lists)]
    for _ in range(steps):
        o.steps(1)
        lists = o.get_lists(0)
        longest.append(max(len(r) for r in lists))
        b = o.best_score()
        if (b != best).any():
            best, best_lists = b.copy(), lists
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists,
                stats=o.stats(), longest=longest)


def _want(spec, r):
    return _oracle_run(tuple(spec["problem"]), spec["seed"] + r, sum(spec["launches"]), spec["max_nearby"], spec["limit"], spec["la"])


def _check(spec, got, mode):
    assert got["mode"] == mode, got["mode"]
    for r, g in enumerate(got["replicas"]):
        w = _want(spec, r)
        assert g["score"] == w["score"], r
        assert g["fresh"] == w["score"], r
        assert g["best"] == w["best"], r
        assert g["lists"] == w["lists"], r
        assert g["best_lists"] == w["best_lists"], r
        for k in ORACLE_WORDS:
            assert g["stats"][k] == w["stats"][k], (r, k)


# ---- 1. row length around a half and a chunk ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,max_nearby", [(8, 5), (8, 20), (8, 64), (31, 20), (32, 20), (33, 20), (34, 20), (63, 20), (64, 20), (65, 20), (66, 20)])
def test_row_length(dim, max_nearby):
    """dim = customers + 1 entries per neighbour row, 3 vehicles, a capacity no start route exceeds: the lanes past a row shorter than a half
    are blanked where the key is taken, a row of exactly 32 / 64 entries has no continuation, 33 / 65 one of a single entry."""
    spec = _spec(_key(dim - 1, 3), max_nearby=max_nearby)
    _check(spec, _gpu_run(spec), 5)


# ---- 2. saturated positions: the per-step flag in both directions, and never set -----------------------------------------------------------
SAT_KEY = _key(200, 300, capacity=600, seed=3, fold=128)  # 300 routes: 7 position bits, pmax = 127; the last route starts with 128 elements


def test_saturation_flag_both_ways():
    """More than 254 routes (pmax = 127) and one route of 128 elements whose length crosses pmax during the solve: the count of routes
    longer than pmax is set at the load, falls to zero and rises again at commits (asserted on the oracle's step-by-step run first), and
    the pass reads the node table in its short form exactly while the count is zero."""
    spec = _spec(SAT_KEY, launches=(20, 30))
    pmax = 127
    for r in range(spec["replicas"]):
        longest = _want(spec, r)["longest"]
        assert longest[0] > pmax
        below = [i for i, n in enumerate(longest) if n <= pmax]
        assert below, longest
        assert any(n > pmax for n in longest[below[0]:]), longest  # ... and back above it afterwards
    _check(spec, _gpu_run(spec), 5)


def test_saturation_flag_never_set():
    """The same 300 routes with no long one: no route reaches pmax during the solve (asserted on the oracle's run)."""
    spec = _spec(_key(200, 300, capacity=55), launches=(20, 30))
    for r in range(spec["replicas"]):
        assert max(_want(spec, r)["longest"]) < 127
    _check(spec, _gpu_run(spec), 5)


# ---- 3. ties -------------------------------------------------------------------------------------------------------------------------------
def _widest_group(key):
    """Entries of the widest equal-distance group over all neighbour rows."""
    return max(int(np.unique(row, return_counts=True)[1].max()) for row in _problem(key)["matrix"])


@pytest.mark.parametrize("customers,vehicles,coord_range,wider_than,narrower_than",
                         [(40, 4, 4, 16, 32), (100, 10, 4, 32, 64), (150, 10, 4, 64, 1 << 30), (100, 10, 30, 1, 32)])
def test_ties(customers, vehicles, coord_range, wider_than, narrower_than):
    """Coordinates on a 4 x 4 grid: 16 distinct points, so rows of a few wide equal-distance groups -- the widest 24 entries at 40 customers,
    55 at 100 (wider than a half: the pass leaves its group open and gen_rest continues it) and 79 at 150 (wider than a chunk: the serial
    top-k, with the rank-only table's 28-bit key), the inversion loop over long runs in all of them.  A 30 x 30 grid at 100 customers:
    many narrow groups.  The widths are asserted on the matrix first."""
    key = _key(customers, vehicles, coord_range=coord_range)
    assert wider_than < _widest_group(key) < narrower_than
    spec = _spec(key)
    _check(spec, _gpu_run(spec), 5)


# ---- 4. max_nearby around the ring sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nearby", [1, 31, 32, 33, 64])
def test_max_nearby(max_nearby):
    """70 customers on 7 vehicles: the small ring up to max_nearby 32, the large one from 33 on, 64 = a whole chunk per source."""
    spec = _spec(_key(70, 7, capacity=55), max_nearby=max_nearby)
    _check(spec, _gpu_run(spec), 5)


# ---- 5. one leaf running dry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [256, 4])
def test_one_leaf_runs_dry(limit):
    """5 customers on 2 vehicles: the leaves run out of sources at different times, so the single-leaf path (leaf 1's key rotated back by 32
    lanes, blanked by the whole lane index) fills the rings; with limit 4 the step usually ends before that, with 256 never."""
    spec = _spec(_key(5, 2, capacity=30), replicas=3, limit=limit, launches=(20, 20))
    _check(spec, _gpu_run(spec), 5)


# ---- 6. every FAST + SMALL instantiation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,mode", MODES, ids=["no_compact", "wpe4", "wpe5", "default", "node_global"])
def test_every_instantiation(env, mode):
    """The dim = 33 row case and the 100-customer tie case under each mode's environment switches, each in a child of its own.  These reach
    launch modes 2, 2, 4, 5 and 6: a model this small has room for 16 wide slices per CU, so capped at 4 waves per SIMD it runs launch mode 2
    again, not 3.  Launch mode 3 (the fifth instantiation) needs a model too large for these shapes: test_compact_slice_at_four_waves."""
    for key in (_key(32, 3), _key(100, 10, coord_range=4)):
        spec = _spec(key)
        _check(spec, _child_run(spec, env), mode)


def test_compact_slice_at_four_waves():
    """Launch mode 3 (the COMPACT slice compiled for 4 waves per SIMD) is taken only by a model too large for 16 wide slices per CU:
    1500 customers on a 30 x 30 grid (ties in every row), a few steps."""
    spec = _spec(_key(1500, 100, capacity=55, seed=4, coord_range=30), launches=(6, 6))
    _check(spec, _child_run(spec, {"SF_AMD_WAVE_WPE": "4"}), 3)


if __name__ == "__main__":  # the child: one run, its results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps(_gpu_run(json.loads(sys.argv[1]))))
