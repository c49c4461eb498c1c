"""GPU parity tests of what the wave engine's FAST + SMALL kernels do once per step and once per source entity, at the smallest
shapes at which each piece can go wrong: the LateAcceptance history slot across launches of every length around the history's size (and a
launch that ends on its move budget mid-window), explicit step seeds that run out inside a launch and on a launch boundary, the entity
order tables at list counts on every side of their 64-entry chunks and of the coprime-mask gate (V <= 128), resolve()'s per-entity path
(lists of 1, 2, 63, 64, 65 and 130 elements, runs of 3 and of 70 empty lists, a list longer than the 16-bit table's position field), and the
deferred best-solution snapshot at element totals on both sides of its 64-lane chunks and of four chunks (255 / 256 / 257), under the
caller's and under the internal node numbering.

The method is that of test_gpu_wave_replay_batch.py: every case asserts the launch mode (sf_list_wave_layout), then compares a fused
multi-launch solve with the CPU oracle bit for bit, replica by replica: working score, fresh score, best score, working lists, best lists
and the seven counters the oracle keeps.  The oracle is stepped one step at a time and its lists are recorded whenever its best score
improves.  What a case rests on (a snapshot really taken mid-launch, a budget that really ends a launch mid-window) is asserted on the
oracle first.

The history and snapshot cases run again under every mode switch, once on the two-level unit and once on the four-level unit.  The
four-level runs use the same CVRP declared with three score levels, the third fed by no constraint (_padded_cvrp): plan_wave_launch takes
launch_tu_list_wave<4> for it, and since a level that is always zero changes no lexicographic comparison its search must equal the
two-level oracle's on the first two levels, lists and counters included.

SF_AMD_NO_COMPACT, SF_AMD_WAVE_WPE and SF_AMD_NODE_GLOBAL are read once per process, so runs under them happen in a fresh child process
(this file run as a script: it prints its results as JSON), one child per mode for all of that mode's specs."""
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
MODE_IDS = ["no_compact", "wpe4", "wpe5", "default", "node_global"]

_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


# ---- problems (built from a hashable key: the oracle's runs are cached per key) ----------------------------------------------------
def _problem(key):
    """key = (customers, vehicles, capacity, seed, lengths): `lengths` None = the round-robin start, else the start lists' lengths in order
    (they sum to `customers`), filled with the customers in ascending order."""
    from solverforge_amd import datasets

    customers, vehicles, capacity, seed, lengths = key
    p = datasets.make_cvrp(customers, vehicles, capacity, seed=seed)
    if lengths is not None:
        assert len(lengths) == vehicles and sum(lengths) == customers
        it = iter(range(1, customers + 1))
        p["routes"] = [[next(it) for _ in range(n)] for n in lengths]
    return p


def _key(customers, vehicles, capacity=55, seed=3, lengths=None):
    return (customers, vehicles, capacity, seed, None if lengths is None else tuple(lengths))


def _spec(problem, replicas=2, seed=5, launches=(15, 20), la=400, limit=256, n_explicit=0, budget=None, renumber=None, levels=2):
    """One fused solve.  `launches`: steps per sf_solve_steps launch; `budget` = (launch index, candidates): that launch is an sf_solve_moves
    launch of at most launches[i] steps.  n_explicit: explicit step seeds for the first n draws of every replica.  renumber: SF_AMD_RENUMBER.
    levels: the model's score levels -- 3 = the same CVRP with one more, least-significant level that no constraint feeds (_padded_cvrp): it
    runs on the four-level unit."""
    return dict(problem=list(problem), replicas=replicas, seed=seed, launches=list(launches), la=la, limit=limit, n_explicit=n_explicit,
                budget=None if budget is None else list(budget), renumber=renumber, levels=levels)


def _step_seeds(spec):
    rng = np.random.default_rng(4321 + spec["n_explicit"])
    return rng.integers(0, 1 << 63, size=(spec["replicas"], spec["n_explicit"]), dtype=np.uint64) * np.uint64(2) + np.uint64(1)


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------
def _padded_cvrp(p, R, levels):
    """models.build_cvrp's model (its three constraints on levels 0 and 1, its two nearby leaves) under `levels` > 2 score levels, the added
    ones fed by nothing.  plan_wave_launch takes the four-level unit for it (three levels run with one more padded level); a level that is
    always zero changes no lexicographic comparison, so the search is the two-level model's, step for step."""
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd.models import FACT_CUSTOMERS, FACT_DEMAND, FACT_MATRIX

    d = GpuScoreDirector(score_levels=levels, hard_levels=1, n_replicas=R)
    d.add_entity_class(0, len(p["routes"]))
    d.add_list_variable(0, p["routes"], element_capacity=len(p["customers"]), element_id_bound=p["matrix"].shape[0])
    d.add_fact_matrix(FACT_MATRIX, p["matrix"])
    d.add_fact_column_i32(FACT_DEMAND, p["demands"])
    d.add_fact_column_u32(FACT_CUSTOMERS, p["customers"])
    d.add_constraint(ConstraintKind.NOT_EXISTS_FLATTENED, 0, fact=FACT_CUSTOMERS, level=0, weight=1)
    d.add_constraint(ConstraintKind.ROUTE_CAPACITY, 0, fact=FACT_DEMAND, param=int(p["capacity"]), level=0, weight=1)
    d.add_constraint(ConstraintKind.ROUTE_DISTANCE, 0, fact=FACT_MATRIX, param=int(p["depot"]), level=1, weight=1)
    d.add_selector(SelectorKind.NEARBY_LIST_CHANGE, 0, max_nearby=20, fact_meter=FACT_MATRIX)
    d.add_selector(SelectorKind.NEARBY_LIST_SWAP, 0, max_nearby=20, fact_meter=FACT_MATRIX)
    return d


def _planned_unit(spec):
    """The instantiation launch_tu_list_wave<L> that plan_wave_launch names for the spec's model (sf_debug_wave_plan: the launch calls the
    same function with the context's level count).  Only `levels` decides it; the shape is the spec's own all the same."""
    import ctypes

    from solverforge_amd import _lib

    customers, vehicles = spec["problem"][0], spec["problem"][1]
    # WaveShape / WaveKnobs / WavePlan as int32 arrays in declaration order (sf_wave_plan.h), as tests/test_wave_plan.py passes them
    shape = [1, vehicles, customers, customers + 1, 20, spec["levels"], 1, 1, 1, 1, 1, 0, 3, 0, 2, 16, 32, spec["replicas"], 0]
    knobs = [0, 6, 4, -1]
    fn = ctypes.CDLL(_lib.LIB_PATH).sf_debug_wave_plan
    fn.restype = ctypes.c_int32
    out, msg, fits = (ctypes.c_int32 * 12)(), ctypes.c_char_p(), (ctypes.c_int32 * 2)()
    rc = fn((ctypes.c_int32 * len(shape))(*shape), len(shape), (ctypes.c_int32 * 4)(*knobs), 4, out, 12, ctypes.byref(msg), fits)
    assert rc == 0, (rc, msg.value)
    return out[1]


def _gpu_run(spec):
    import solverforge_amd as sfa

    p = _problem(tuple(spec["problem"][:4]) + (None if spec["problem"][4] is None else tuple(spec["problem"][4]),))
    R = spec["replicas"]
    before = os.environ.get("SF_AMD_RENUMBER")
    if spec["renumber"] is not None:
        os.environ["SF_AMD_RENUMBER"] = spec["renumber"]  # (read per model, at sf_initialize)
    try:
        d = sfa.build_cvrp(p, n_replicas=R) if spec["levels"] == 2 else _padded_cvrp(p, R, spec["levels"])
        d.set_engine(2)
        d.configure(sfa.SolverConfig(late_acceptance_size=spec["la"], accepted_count_limit=spec["limit"], random_seed=spec["seed"]))
        if spec["n_explicit"]:
            d.set_step_seeds(_step_seeds(spec))
        d.calculate_score()
    finally:
        if spec["renumber"] is not None:
            if before is None:
                del os.environ["SF_AMD_RENUMBER"]
            else:
                os.environ["SF_AMD_RENUMBER"] = before
    d.phase_start()
    for i, n in enumerate(spec["launches"]):
        if spec["budget"] and spec["budget"][0] == i:
            d.solve_moves(n, spec["budget"][1])
        else:
            d.solve_steps(n)
    mode, renumbered = d.wave_layout()
    score, best = d.calculate_score(), d.best_scores()
    fresh = d.fresh_score()
    out = dict(mode=mode, renumbered=renumbered, levels=d.levels, replicas=[])
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
def _oracle_run(problem, replica_seed, launches, la, limit, seeds, budget):
    """One replica through the launches.  Scores, lists, counters at the end; the best lists as they were when the best score last improved;
    `launch_steps` = the steps each launch ran (a budgeted launch ends after the step in which the candidates it generated reach the budget)."""
    sfo = _SFO["sfo"]
    p = _problem(problem)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=la, limit=limit, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=20, random_seed=replica_seed)
    if seeds:
        o.set_step_seeds(np.array(seeds, dtype=np.uint64))
    o.phase_start()
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    launch_steps, improved_at, step = [], [], 0
    for i, n in enumerate(launches):
        at_start = o.stats()["moves_generated"]
        ran = 0
        for _ in range(n):
            o.steps(1)
            ran += 1
            step += 1
            b = o.best_score()
            if (b != best).any():
                best, best_lists = b.copy(), o.get_lists(0)
                improved_at.append(step)
            if budget is not None and budget[0] == i and o.stats()["moves_generated"] - at_start >= budget[1]:
                break
        launch_steps.append(ran)
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists,
                stats=o.stats(), launch_steps=launch_steps, improved_at=improved_at)


def _want(spec, r):
    seeds = tuple(int(x) for x in _step_seeds(spec)[r]) if spec["n_explicit"] else None
    pk = tuple(spec["problem"][:4]) + (None if spec["problem"][4] is None else tuple(spec["problem"][4]),)
    return _oracle_run(pk, spec["seed"] + r, tuple(spec["launches"]), spec["la"], spec["limit"], seeds, None if spec["budget"] is None else tuple(spec["budget"]))


def _check(spec, got, mode):
    assert got["mode"] == mode, got["mode"]
    pad = [0] * (spec["levels"] - 2)  # (the padded levels: nothing feeds them)
    assert got["levels"] == spec["levels"] and _planned_unit(spec) == (2 if spec["levels"] <= 2 else 4)
    if spec["renumber"] is not None and mode >= 3:
        assert got["renumbered"] == (spec["renumber"] == "1")
    for r, g in enumerate(got["replicas"]):
        w = _want(spec, r)
        assert g["score"] == w["score"] + pad, r
        assert g["fresh"] == w["score"] + pad, r  # fresh equals incremental
        assert g["best"] == w["best"] + pad, r
        assert g["lists"] == w["lists"], r
        assert g["best_lists"] == w["best_lists"], r
        for k in ORACLE_WORDS:
            assert g["stats"][k] == w["stats"][k], (r, k)


def _rescore(spec, lists):
    """Score of `lists` computed from scratch by the oracle."""
    sfo = _SFO["sfo"]
    p = _problem(tuple(spec["problem"][:4]) + (None if spec["problem"][4] is None else tuple(spec["problem"][4]),))
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], [list(x) for x in lists])
    return [int(x) for x in o.score()[:2]]


# ---- 1. the LateAcceptance history slot ---------------------------------------------------------------------------------------------------
HIST_KEY = _key(40, 4)
LA_SIZES = [1, 2, 3, 5]


def _history_specs(la):
    """Three launches in a row of 1, 2, la, la + 1 and 2 la + 1 steps each: the cursor wraps inside a launch, on a launch's last step and
    not at all; the slot a step reads was written by the step before (la 1), by the commit before that (la 2), or launches ago."""
    return [_spec(HIST_KEY, replicas=4, launches=(n, n, n), la=la) for n in sorted({1, 2, la, la + 1, 2 * la + 1})]


@pytest.mark.parametrize("la", LA_SIZES)
def test_history_slot_across_launches(la):
    for spec in _history_specs(la):
        _check(spec, _gpu_run(spec), 5)


def _budget_spec(la):
    # 600 candidates: two or three steps of up to 256 pulls each; then a fixed-step launch that goes on from the cursor the budget left
    return _spec(HIST_KEY, replicas=4, launches=(50, 2 * la + 1), la=la, budget=(0, 600))


@pytest.mark.parametrize("la", [3, 5])
def test_budget_ends_a_launch_mid_window(la):
    """An sf_solve_moves launch that its budget ends (asserted on the oracle: well before its 50 steps) with the history cursor inside the
    window for at least one replica (steps not a multiple of the history's size), followed by a fixed-step launch."""
    spec = _budget_spec(la)
    ran = [_want(spec, r)["launch_steps"][0] for r in range(spec["replicas"])]
    assert all(0 < n < 50 for n in ran), ran
    assert any(n % la for n in ran), ran
    got = _gpu_run(spec)
    _check(spec, got, 5)
    for r, g in enumerate(got["replicas"]):
        assert g["stats"]["step_count"] == sum(_want(spec, r)["launch_steps"]), r


# ---- 2. explicit step seeds that run out ----------------------------------------------------------------------------------------------------------
SEED_LAUNCHES = (6, 7)


@pytest.mark.parametrize("n_explicit", [0, 1, SEED_LAUNCHES[0] - 1, SEED_LAUNCHES[0], SEED_LAUNCHES[0] + 3])
def test_explicit_seeds_run_out(n_explicit):
    """sf_solver_set_step_seeds with 0, 1, steps - 1, steps and steps + 3 seeds against launches of 6 and 7 steps: the draw that crosses to
    hashed seeds is the first of all, the second, the last of the first launch, the first of the second launch, and its fourth."""
    spec = _spec(HIST_KEY, replicas=3, launches=SEED_LAUNCHES, n_explicit=n_explicit)
    _check(spec, _gpu_run(spec), 5)


# ---- 3. the entity order tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 3, 63, 64, 65, 127, 128, 129])
def test_order_tables(V):
    """Two customers per list plus three: list counts of one table chunk less one, exactly one, one more, two chunks around 128 -- and both
    sides of the coprime-mask gate (V <= 128: the lane-parallel hashes; V = 129: the scalar permutation parameters).  V = 2: the stride's
    divisor V - 1 is 1."""
    spec = _spec(_key(2 * V + 3, V, capacity=20), launches=(8, 8))
    _check(spec, _gpu_run(spec), 5)


# ---- 4. resolve()'s per-entity path ----------------------------------------------------------------------------------------------------------------
ENTITY_LENGTHS = [1] + [0] * 3 + [2] + [0] * 70 + [63, 64, 65, 130]  # 79 lists: runs of three and of seventy empty lists between occupied ones
LONG_LENGTHS = [1] + [0] * 3 + [2] + [0] * 70 + [63, 64, 65, 520]    # 79 lists: 7 route bits, 9 position bits -- 520 > pmax = 511


def test_entity_lengths_and_empty_runs():
    """Lists of 1, 2, 63, 64, 65 and 130 elements (a list of one: the remainder's divisor 1; 64 / 65 / 130: one, two and three 64-offset
    chunks of sources), with runs of 3 and of 70 empty lists for resolve()'s skip loop to cross."""
    spec = _spec(_key(sum(ENTITY_LENGTHS), len(ENTITY_LENGTHS), capacity=400, lengths=ENTITY_LENGTHS), launches=(6, 6))
    _check(spec, _gpu_run(spec), 5)


@pytest.mark.parametrize("n", [0, 3], ids=["no_compact", "default"])
def test_a_list_longer_than_the_position_field(n):
    """One list of 520 elements on 79 lists -- longer than the 511 positions the COMPACT table's field holds: in the wide layout (launch
    mode 2) it is a list like any other, in the COMPACT one (launch mode 5) its tail is found by the saturation scan."""
    spec = _spec(_key(sum(LONG_LENGTHS), len(LONG_LENGTHS), capacity=2000, lengths=LONG_LENGTHS), launches=(5, 5))
    (got,) = _child_run([spec], MODES[n][0])
    _check(spec, got, MODES[n][1])


# ---- 5. the deferred best-solution snapshot ----------------------------------------------------------------------------------------------------
SNAP_TOTALS = [63, 64, 65, 255, 256, 257]
SNAP_LIMIT = 2
SNAP_SEED = {63: 5, 64: 7, 65: 5, 255: 5, 256: 5, 257: 7}  # solver seeds at which both replicas end the launch off their best state (asserted)


def _snapshot_spec(total, renumber):
    # (AcceptedCount 2: the forager picks among the first two accepted candidates, and the history -- still at the start's score -- accepts
    # nearly all, so the search steps off its best state again and again within the launch; at 256 every one of the first 60 steps improves)
    return _spec(_key(total, max(2, total // 10)), seed=SNAP_SEED[total], launches=(60,), limit=SNAP_LIMIT, renumber=renumber)


def _assert_snapshot_taken_mid_launch(spec):
    for r in range(spec["replicas"]):
        w = _want(spec, r)
        assert w["improved_at"] and w["best"] != w["score"], (r, w["best"], w["score"])  # the search left its best state: the snapshot was written mid-launch


@pytest.mark.parametrize("renumber", ["0", "1"], ids=["caller_ids", "internal_ids"])
@pytest.mark.parametrize("total", SNAP_TOTALS)
def test_snapshot(total, renumber):
    """60 steps from the round-robin start in one launch: the best score improves and the search then leaves that state (asserted on the
    oracle), so the kernel wrote the snapshot inside its step loop: `total` elements in chunks of 64 lanes, each element through the inverse
    numbering when the model is renumbered.  The best lists, re-scored from scratch, carry the best score."""
    spec = _snapshot_spec(total, renumber)
    _assert_snapshot_taken_mid_launch(spec)
    got = _gpu_run(spec)
    _check(spec, got, 5)
    for g in got["replicas"]:
        assert _rescore(spec, g["best_lists"]) == g["best"]


# ---- 6. every FAST + SMALL instantiation ---------------------------------------------------------------------------------------------------------
def _instantiation_specs(levels):
    """Every history case (all launch lengths, both budget cases) and every snapshot case (all six totals, both numberings)."""
    hist = [s for la in LA_SIZES for s in _history_specs(la)] + [_budget_spec(la) for la in (3, 5)]
    snap = [_snapshot_spec(t, rn) for t in SNAP_TOTALS for rn in ("0", "1")]
    return [dict(s, levels=levels) for s in hist + snap]


UNITS = [2, 3]  # score levels of the model: 2 = the two-level unit, 3 = the padded model on the four-level unit (_padded_cvrp)
UNIT_IDS = ["two_level", "four_level"]


@pytest.mark.parametrize("n", range(len(MODES)), ids=MODE_IDS)
@pytest.mark.parametrize("levels", UNITS, ids=UNIT_IDS)
def test_every_instantiation(levels, n):
    """The history and snapshot cases under each mode's switches, on the two-level and on the four-level unit: one child process per mode
    and unit.  These reach launch modes 2, 2, 4, 5 and 6 of launch_tu_list_wave<2> and <4>.  The four-level runs are compared with the same
    two-level oracle: first two levels equal, the padded one zero."""
    specs = _instantiation_specs(levels)
    for spec in specs:
        if spec["renumber"] is not None:
            _assert_snapshot_taken_mid_launch(spec)
    pad = [0] * (levels - 2)
    for spec, got in zip(specs, _child_run(specs, MODES[n][0])):
        _check(spec, got, MODES[n][1])
        if spec["renumber"] is not None:
            for g in got["replicas"]:
                assert _rescore(spec, g["best_lists"]) + pad == g["best"]


@pytest.mark.parametrize("levels", UNITS, ids=UNIT_IDS)
def test_compact_slice_at_four_waves(levels):
    """Launch mode 3 (the COMPACT slice compiled for 4 waves per SIMD) is taken only by a model too large for 16 wide slices per CU: 1500
    customers on 100 lists, a history of 3 over launches of 3, 4 and 7 steps -- on both units."""
    spec = _spec(_key(1500, 100), launches=(3, 4, 7), la=3, levels=levels)
    (got,) = _child_run([spec], {"SF_AMD_WAVE_WPE": "4"})
    _check(spec, got, 3)


if __name__ == "__main__":  # the child: its runs one after another, their results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps([_gpu_run(s) for s in json.loads(sys.argv[1])]))
