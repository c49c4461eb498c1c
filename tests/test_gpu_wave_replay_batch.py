"""GPU parity tests of the replay batch of the wave engine's FAST + SMALL kernels at the smallest shapes at which its register-level
paths can go wrong.  Launch modes 2 - 5 have the lean batch; launch mode 6 (the node table in HBM) keeps the batch it had, so its
cases here run unchanged code and serve as the independent reference for candidates_scored, the one counter whose computation the lean batch
restructures and the oracle does not keep.  Covered: the AcceptedCount cut at every lane edge of a 64-wide batch (the cut is computed only in the batch
whose accepted lanes reach the quota), the cut among rejected candidates, the two-level score key at the largest weights the 32-bit host
gate admits (hard deltas of both signs under negative soft deltas: the borrow between the key's two words) and with a constraint
weighted zero, every pattern of the trial delta (single-element sources, empty destinations, adjacent intra-list swaps, equal
distances), one leaf running dry (batches with all 64 lanes on one leaf, a leaf's last batch shorter than 64), LateAcceptance histories
of 1 and 400 entries, all five instantiations, and candidates_scored equal across them.

The method is that of test_gpu_wave_paired_pass.py: every case asserts the launch mode first (sf_list_wave_layout), then compares a
fused multi-launch solve with the CPU oracle bit for bit, replica by replica: working score, best score, fresh score, working lists,
best lists and the seven counters the oracle keeps.  The oracle is stepped one step at a time and its lists are recorded whenever its
best score improves.  Preconditions a case rests on (every candidate accepted, a step that ends dry) are asserted on the oracle's
counters first.

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

    customers, vehicles, capacity, seed, fold, coord_range, singles = key
    p = datasets.make_cvrp(customers, vehicles, capacity, seed=seed, coord_range=coord_range)
    if fold or singles:  # `fold` empty routes at the start, then `singles` routes of one element, the other customers dealt over the rest
        order = [c for r in p["routes"] for c in r]
        routes = [[] for _ in range(vehicles)]
        for v in range(fold, fold + singles):
            routes[v] = [order.pop(0)]
        rest = vehicles - fold - singles
        for n, c in enumerate(order):
            routes[fold + singles + n % rest].append(c)
        p["routes"] = routes
    return p


def _key(customers, vehicles, capacity=10_000, seed=3, fold=0, coord_range=1000, singles=0):
    return (customers, vehicles, capacity, seed, fold, coord_range, singles)


def _spec(problem, weights=(1, 1, 1), replicas=2, seed=5, launches=(15, 20), max_nearby=20, limit=256, la=400):
    return dict(problem=list(problem), weights=list(weights), replicas=replicas, seed=seed, launches=list(launches), max_nearby=max_nearby, limit=limit, la=la)


def _largest_weights(key):
    """The largest capacity and distance weights the host gate of the 32-bit trial arithmetic admits for this problem (sf_api.hip):
    weight x 2 x (sum of demands + capacity + 1) < 2^29 and weight x 8 x (longest leg + 1) < 2^29."""
    p = _problem(key)
    dem = int(np.abs(p["demands"].astype(np.int64)).sum())
    cw = ((1 << 29) - 1) // (2 * (dem + int(p["capacity"]) + 1))
    dw = ((1 << 29) - 1) // (8 * (int(p["matrix"].max()) + 1))
    assert cw * 2 * (dem + int(p["capacity"]) + 1) < 1 << 29 <= (cw + 1) * 2 * (dem + int(p["capacity"]) + 1)
    assert dw * 8 * (int(p["matrix"].max()) + 1) < 1 << 29 <= (dw + 1) * 8 * (int(p["matrix"].max()) + 1)
    return cw, dw


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------
def _gpu_run(spec):
    import solverforge_amd as sfa

    p = _problem(tuple(spec["problem"]))
    R = spec["replicas"]
    d = sfa.build_cvrp(p, n_replicas=R, max_nearby=spec["max_nearby"], weights=tuple(spec["weights"]))
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


def _child_run(specs, env):
    """The specs one after another in ONE fresh child process under `env`; a result per spec."""
    e = {k: v for k, v in os.environ.items() if k not in MODE_ENVS}
    e.update(env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(specs)], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


# ---- the oracle's run ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(problem, weights, replica_seed, steps, max_nearby, limit, la):
    """Scores, lists and counters after `steps` steps of one replica."""
    sfo = _SFO["sfo"]
    p = _problem(problem)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=weights)
    o.configure(la_size=la, limit=limit, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=max_nearby, random_seed=replica_seed)
    o.phase_start()
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    hard = [int(o.score()[0])]
    for _ in range(steps):
        o.steps(1)
        hard.append(int(o.score()[0]))
        b = o.best_score()
        if (b != best).any():
            best, best_lists = b.copy(), o.get_lists(0)
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists,
                stats=o.stats(), hard=hard)


def _want(spec, r):
    return _oracle_run(tuple(spec["problem"]), tuple(spec["weights"]), spec["seed"] + r, sum(spec["launches"]), spec["max_nearby"], spec["limit"], spec["la"])


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


# ---- 1. the AcceptedCount cut, every edge ------------------------------------------------------------------------------------------------
FLAT_KEY = _key(40, 4)  # a capacity no route exceeds: with the distance weighted zero every trial delta is zero
CUT_LIMITS = [1, 2, 32, 33, 63, 64, 65, 127, 128, 129, 256]


def _flat_spec(limit):
    return _spec(FLAT_KEY, weights=(1, 1, 0), limit=limit)


def _assert_every_candidate_accepted(spec):
    steps = sum(spec["launches"])
    for r in range(spec["replicas"]):
        st = _want(spec, r)["stats"]
        assert st["moves_accepted"] == st["moves_evaluated"] == steps * spec["limit"], (r, st)


@pytest.mark.parametrize("limit", CUT_LIMITS)
def test_cut_every_edge(limit):
    """weights (1, 1, 0) and a capacity that is never exceeded: every candidate is accepted (asserted on the oracle's counters: accepted ==
    evaluated == steps x limit), so a step ends exactly at its limit-th pull -- in lane 0 (1, 65, 129), mid-batch (2, 32, 33, 63, 127), in
    lane 63 with exactly 64 remaining (64, 128, 256).  Every accepted candidate ties, so the forager's equal count runs across batches far
    above 64 and the reservoir pick draws in every one."""
    spec = _flat_spec(limit)
    _assert_every_candidate_accepted(spec)
    _check(spec, _gpu_run(spec), 5)


# ---- 2. the cut with rejections ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1, 1, 1), (1, 1, 7)], ids=["w1", "w7"])
@pytest.mark.parametrize("limit", [1, 64, 65, 256])
def test_cut_with_rejections(weights, limit):
    """The same model with the distance counted: some candidates are rejected (asserted for the limits of a batch and more), so the lane
    that reaches the quota is not the limit-th lane and the batch that holds it is not the (limit / 64)-th."""
    spec = _spec(FLAT_KEY, weights=weights, limit=limit)
    for r in range(spec["replicas"]):
        st = _want(spec, r)["stats"]
        assert st["moves_accepted"] <= st["moves_evaluated"]
        if limit >= 64:
            assert st["moves_accepted"] < st["moves_evaluated"], st
    _check(spec, _gpu_run(spec), 5)


# ---- 3. the score key ------------------------------------------------------------------------------------------------------------------------------
TIGHT_KEY = _key(60, 6, capacity=55)  # ten customers of demand 1 .. 9 per route against a capacity of 55: routes on both sides of it


def _key_weights():
    cw, dw = _largest_weights(TIGHT_KEY)
    return [(1, 1, dw), (1, cw, 1), (1, cw, 7), (1, cw, dw), (1, 0, 1), (1, 0, dw)]


@pytest.mark.parametrize("case", range(6), ids=["dist_max", "cap_max", "cap_max_dist7", "both_max", "cap_zero", "cap_zero_dist_max"])
def test_key_weights(case):
    """The largest weights the 32-bit gate admits (launch mode 5 is asserted: the gate did admit them), on a model whose routes sit on both
    sides of the capacity: hard deltas of both signs while most soft deltas are negative -- the borrow between the two words of the
    64-bit key --, and level deltas next to 2^29.  The oracle's hard score must move during the solve (asserted) for the capacity cases.
    Capacity weight zero: a constraint that exists and feeds nothing."""
    weights = _key_weights()[case]
    spec = _spec(TIGHT_KEY, weights=weights)
    if weights[1]:
        assert any(len(set(_want(spec, r)["hard"])) > 1 for r in range(spec["replicas"]))
    _check(spec, _gpu_run(spec), 5)


# ---- 4. patterns of the trial delta --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coord_range,capacity", [(6, 10_000), (6, 12), (1000, 12)])
def test_delta_patterns(coord_range, capacity):
    """40 customers on 12 vehicles: four empty routes, four of a single element, the rest on four routes -- the change out of a one-element
    list (no closing leg), the change into an empty list (no opened leg), and adjacent intra-list swaps; a 6 x 6 grid makes equal
    distances, hence zero deltas and ties, common; capacity 12 puts the hard level into play."""
    spec = _spec(_key(40, 12, capacity=capacity, fold=4, singles=4, coord_range=coord_range))
    p = _problem(tuple(spec["problem"]))
    assert sorted(len(r) for r in p["routes"])[:8] == [0] * 4 + [1] * 4
    _check(spec, _gpu_run(spec), 5)


# ---- 5. one leaf running dry, LateAcceptance histories of 1 and 400 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("la,max_nearby", [(1, 5), (1, 20), (400, 5)])
def test_one_leaf_runs_dry(la, max_nearby):
    """With few candidates accepted a step pulls every candidate of both leaves: the leaf with fewer runs dry first, the other goes on alone
    (64 lanes on one leaf), and each leaf's last batch is shorter than 64.  Asserted on the oracle: fewer accepted than steps x limit, so
    steps did end dry."""
    spec = _spec(_key(40, 4, capacity=55), la=la, max_nearby=max_nearby)
    steps = sum(spec["launches"])
    for r in range(spec["replicas"]):
        assert _want(spec, r)["stats"]["moves_accepted"] < steps * spec["limit"]
    _check(spec, _gpu_run(spec), 5)


def test_history_of_one_with_every_candidate_accepted():
    """late_acceptance_size 1 on the flat model, limit 65: the late score is the last step's score in every step."""
    spec = dict(_flat_spec(65), la=1)
    _assert_every_candidate_accepted(spec)
    _check(spec, _gpu_run(spec), 5)


# ---- 6. every FAST + SMALL instantiation ---------------------------------------------------------------------------------------------------------
def _instantiation_specs():
    return [_flat_spec(64), _flat_spec(65), _spec(FLAT_KEY, weights=(1, 1, 7), limit=64), _spec(TIGHT_KEY, weights=_key_weights()[3])]


_MODE_RUNS = {}


def _mode_run(n):
    """The instantiation specs under MODES[n]'s switches: one child per mode, run once and shared by the tests below."""
    if n not in _MODE_RUNS:
        _MODE_RUNS[n] = _child_run(_instantiation_specs(), MODES[n][0])
    return _MODE_RUNS[n]


@pytest.mark.parametrize("n", range(len(MODES)), ids=["no_compact", "wpe4", "wpe5", "default", "node_global"])
def test_every_instantiation(n):
    """The cut in lane 63 and in lane 0 of a batch (limits 64 and 65 on the flat model), the cut with rejections at (1, 1, 7), and the
    largest key weights, under each mode's environment switches, in one child of its own per mode.  These reach launch modes 2, 2, 4, 5
    and 6; launch mode 3 needs a larger model: test_compact_slice_at_four_waves."""
    specs = _instantiation_specs()
    _assert_every_candidate_accepted(specs[0])
    _assert_every_candidate_accepted(specs[1])
    for spec, got in zip(specs, _mode_run(n)):
        _check(spec, got, MODES[n][1])


def test_candidates_scored_same_in_every_instantiation():
    """candidates_scored (every candidate a batch priced, consumed or not) and sources_scanned are not kept by the oracle.  The lean batch
    adds candidates_scored once per step from the pulls, plus the cut batch's priced-but-not-consumed remainder; launch mode 6 still adds
    it batch by batch.  The same solves must give the same words in both forms, replica by replica -- and more scored than evaluated
    wherever the cut leaves a remainder (limit 65 on the flat model: one lane consumed of a full second batch)."""
    specs = _instantiation_specs()
    ref = _mode_run(len(MODES) - 1)  # node_global: launch mode 6, the per-batch form
    assert ref[0]["mode"] == 6
    for n in range(len(MODES) - 1):
        got = _mode_run(n)
        assert got[0]["mode"] in (2, 4, 5)
        for spec, g, w in zip(specs, got, ref):
            for r in range(spec["replicas"]):
                for k in ("candidates_scored", "sources_scanned"):
                    assert g["replicas"][r]["stats"][k] == w["replicas"][r]["stats"][k], (n, spec["limit"], r, k)
    for r in range(specs[1]["replicas"]):
        st = ref[1]["replicas"][r]["stats"]
        assert st["candidates_scored"] > st["moves_evaluated"], st


def test_compact_slice_at_four_waves():
    """Launch mode 3 (the COMPACT slice compiled for 4 waves per SIMD) is taken only by a model too large for 16 wide slices per CU: 1500
    customers on a 30 x 30 grid, a few steps -- once with every candidate accepted and the cut at lane 0 of the second batch, once with
    the largest key weights."""
    key = _key(1500, 100, capacity=55, seed=4, coord_range=30)
    cw, dw = _largest_weights(key)
    specs = [_spec(_key(1500, 100, seed=4, coord_range=30), weights=(1, 1, 0), limit=65, launches=(6, 6)), _spec(key, weights=(1, cw, dw), launches=(6, 6))]
    _assert_every_candidate_accepted(specs[0])
    for spec, got in zip(specs, _child_run(specs, {"SF_AMD_WAVE_WPE": "4"})):
        _check(spec, got, 3)


if __name__ == "__main__":  # the child: its runs one after another, their results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps([_gpu_run(s) for s in json.loads(sys.argv[1])]))
