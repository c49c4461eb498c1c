"""GPU parity tests of the lockstep round of the wave engine's FAST + SMALL kernels at the smallest shapes at which it can go
wrong.  In launch modes 2 - 5 and in the run-time unit a step starts in the round: one (heads, tails, sources left) triple for both leaves,
paired passes while fewer than 32 candidates per leaf are pending, 64-lane batches without an availability test.  The round ends with the
step at the AcceptedCount cut, or hands its cursors to the general loop when a source emits other than max_nearby candidates or the
sources run out with a batch still short; it is not entered when the two max_nearby differ, exceed 32, or there is nothing to scan.
Launch mode 6 (SF_AMD_NODE_GLOBAL=1) compiles the general loop alone and is the reference inside the same library for what the oracle does
not keep.

Every case is a fused solve of three launches of a few steps.  It runs under SF_AMD_WAVE_SPEC = 0 (the ahead-of-time kernel) and = 1 (the
unit compiled for the context's constants; the switch is read at every launch and sf_debug_wave_spec must say which kernel ran), and every
replica's working, fresh and best score, working and best lists and the oracle's seven counters must equal the CPU oracle's bit for bit;
every LateAcceptance slot, the history cursor and every sf_stats word (candidates_scored and sources_scanned included) must equal the
same solve in launch mode 6.  What a case rests on -- the union's first leaf taking both values, a source that emits fewer than
max_nearby after sources that emitted all of them, steps that scan every source -- is asserted on the oracle's trace first, from the
consumed candidates: a leaf's consecutive pulls with one first operand (list, position) come from one source -- or from two in a row that
read alike, so the groups are tested for multiples of max_nearby.

The two max_nearby can differ on the device only (the oracle's configuration has one for all leaves): that case is compared with launch
mode 6 alone.

SF_AMD_NO_COMPACT, SF_AMD_WAVE_WPE and SF_AMD_NODE_GLOBAL are read once per process, so runs under them happen in a fresh child process
(this file run as a script: it prints its results as JSON), one child per mode for all of that mode's runs."""
import ctypes
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
MODES = {"no_compact": ({"SF_AMD_NO_COMPACT": "1"}, 2), "wpe4": ({"SF_AMD_WAVE_WPE": "4"}, 2), "wpe5": ({"SF_AMD_WAVE_WPE": "5"}, 4), "default": ({}, 5),
         "node_global": ({"SF_AMD_NODE_GLOBAL": "1"}, 6)}
AOT, SPECIALISED, R_KNOB, R_MODE = 0, 1, 1, 2
NEVER = 1 << 20  # an AcceptedCount limit no step reaches: every step scans every source

_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


# ---- problems and specs ---------------------------------------------------------------------------------------------------------------------
def _problem(key):
    """key = (customers, vehicles, capacity, seed, lengths): `lengths` None = the round-robin start, else the start lists' lengths in order,
    filled with the customers in ascending order; customers beyond their sum start unassigned."""
    from solverforge_amd import datasets

    customers, vehicles, capacity, seed, lengths = key
    p = datasets.make_cvrp(customers, vehicles, capacity, seed=seed)
    if lengths is not None:
        assert len(lengths) == vehicles and sum(lengths) <= customers
        it = iter(range(1, customers + 1))
        p["routes"] = [[next(it) for _ in range(n)] for n in lengths]
    return p


def _key(customers, vehicles, capacity=55, seed=3, lengths=None):
    return (customers, vehicles, capacity, seed, None if lengths is None else tuple(lengths))


def _spec(problem, weights=(1, 1, 1), k=20, limit=256, la=400, launches=(5, 4, 6), budget=None, levels=2, replicas=4, seed=5):
    """One fused solve.  k: max_nearby of both leaves, or a pair (change, swap).  budget = (launch index, candidates): that launch is an
    sf_solve_moves launch of at most launches[i] steps.  levels 3: the same CVRP with a third level that nothing feeds (the four-level unit)."""
    k = [k, k] if isinstance(k, int) else list(k)
    return dict(problem=list(problem), weights=list(weights), k=k, limit=limit, la=la, launches=list(launches), budget=None if budget is None else list(budget),
                levels=levels, replicas=replicas, seed=seed)


def _pkey(spec):
    return tuple(spec["problem"][:4]) + (None if spec["problem"][4] is None else tuple(spec["problem"][4]),)


BIG = _key(100, 5)                         # 100 nodes on 5 lists: every source has 20 destinations, the round holds for whole steps
FLAT = _key(100, 5, capacity=10_000)       # ... and with the distance weighted zero every trial delta is zero: every candidate is accepted
FEW = _key(31, 3, lengths=(11, 10, 10))    # 31 elements at max_nearby 1: the sources run out with 31 candidates per leaf pending
CASES = {
    # the round holds for whole steps, to the cut
    "holds_limit8": _spec(BIG, limit=8),
    "holds_limit256": _spec(BIG),
    # max_nearby: 1, 16 (exactly two passes per batch), 20, 32 (one pass per batch); 33 and unequal ones never enter the round
    "k1": _spec(BIG, k=1),
    "k16": _spec(BIG, k=16),
    "k32": _spec(BIG, k=32),
    "k33_not_entered": _spec(BIG, k=33),
    # the quota's cut inside a full batch (test_gpu_wave_replay_batch.py's constructions): lane 0, lane 63 with exactly 64 accepted and 64
    # remaining, mid-batch, and among rejections
    "cut_lane0": _spec(FLAT, weights=(1, 1, 0), limit=65),
    "cut_lane63": _spec(FLAT, weights=(1, 1, 0), limit=64),
    "cut_lane63_second_batch": _spec(FLAT, weights=(1, 1, 0), limit=128),
    "cut_mid_batch": _spec(FLAT, weights=(1, 1, 0), limit=33),
    "cut_among_rejections": _spec(FLAT, weights=(1, 1, 7), limit=64),
    # exits because a source emits fewer than max_nearby, in steps that scan every source
    "exit_first_pass": _spec(_key(12, 3), limit=NEVER),
    "exit_late": _spec(_key(40, 4), limit=NEVER),
    # exits because the sources run out with fewer than 32 pending: 1, 2, 3 and 31 elements (the rest of the 31 customers unassigned)
    "runs_out_1": _spec(_key(31, 3, lengths=(1, 0, 0)), k=1, limit=NEVER),
    "runs_out_2": _spec(_key(31, 3, lengths=(1, 1, 0)), k=1, limit=NEVER),
    "runs_out_3": _spec(_key(31, 3, lengths=(1, 1, 1)), k=1, limit=NEVER),
    "runs_out_31": _spec(FEW, k=1, limit=NEVER),
    # nothing to scan: the round is not entered
    "all_lists_empty": _spec(_key(31, 3, lengths=(0, 0, 0))),
    # runs of empty lists in front of the first entity
    "empty_runs": _spec(_key(100, 12, lengths=[0] * 7 + [20] * 5)),
    # a launch its move budget ends in the middle of the sequence, then a fixed-step one
    "budget_mid_sequence": _spec(BIG, launches=(4, 50, 5), budget=(1, 600)),
    # the four-level unit, through a CVRP declared on three levels
    "four_level_unit": _spec(BIG, levels=3),
}
DEVICE_ONLY = {"k20_k5_not_entered": _spec(BIG, k=(20, 5))}  # (no oracle: compared with launch mode 6)
ALL = dict(CASES, **DEVICE_ONLY)
# the cases every other instantiation runs as well: the round to the cut, the cut's edges, both exits, the budget, the four-level unit
EVERY_MODE = ["holds_limit256", "k16", "k32", "cut_lane0", "cut_lane63", "cut_among_rejections", "exit_late", "runs_out_31", "budget_mid_sequence", "four_level_unit"]


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------
def _director(spec):
    import solverforge_amd as sfa
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd.models import FACT_CUSTOMERS, FACT_DEMAND, FACT_MATRIX

    p = _problem(_pkey(spec))
    d = GpuScoreDirector(score_levels=spec["levels"], hard_levels=1, n_replicas=spec["replicas"])  # models.build_cvrp, with a max_nearby per leaf
    d.add_entity_class(0, len(p["routes"]))
    d.add_list_variable(0, p["routes"], element_capacity=len(p["customers"]), element_id_bound=p["matrix"].shape[0])
    d.add_fact_matrix(FACT_MATRIX, p["matrix"])
    d.add_fact_column_i32(FACT_DEMAND, p["demands"])
    d.add_fact_column_u32(FACT_CUSTOMERS, p["customers"])
    d.add_constraint(ConstraintKind.NOT_EXISTS_FLATTENED, 0, fact=FACT_CUSTOMERS, level=0, weight=spec["weights"][0])
    d.add_constraint(ConstraintKind.ROUTE_CAPACITY, 0, fact=FACT_DEMAND, param=int(p["capacity"]), level=0, weight=spec["weights"][1])
    d.add_constraint(ConstraintKind.ROUTE_DISTANCE, 0, fact=FACT_MATRIX, param=int(p["depot"]), level=1, weight=spec["weights"][2])
    d.add_selector(SelectorKind.NEARBY_LIST_CHANGE, 0, max_nearby=spec["k"][0], fact_meter=FACT_MATRIX)
    d.add_selector(SelectorKind.NEARBY_LIST_SWAP, 0, max_nearby=spec["k"][1], fact_meter=FACT_MATRIX)
    d.set_engine(2)
    d.configure(sfa.SolverConfig(late_acceptance_size=spec["la"], accepted_count_limit=spec["limit"], random_seed=spec["seed"]))
    d.calculate_score()
    d.phase_start()
    return d


def _gpu_run(spec, knob):
    """The solve with every launch under SF_AMD_WAVE_SPEC = knob: the launch mode, what sf_debug_wave_spec said after each launch, and the
    state left behind in every replica."""
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_wave_spec.restype = ctypes.c_int32
    L.sf_debug_late_acceptance.restype = ctypes.c_int32
    d = _director(spec)
    before = os.environ.get("SF_AMD_WAVE_SPEC")
    os.environ["SF_AMD_WAVE_SPEC"] = knob
    said = []
    try:
        for i, n in enumerate(spec["launches"]):
            if spec["budget"] and spec["budget"][0] == i:
                d.solve_moves(n, spec["budget"][1])
            else:
                d.solve_steps(n)
            out = (ctypes.c_int32 * 22)()
            assert L.sf_debug_wave_spec(d._h, out, len(out)) == 0
            said.append([out[0], out[1]])
    finally:
        if before is None:
            os.environ.pop("SF_AMD_WAVE_SPEC", None)
        else:
            os.environ["SF_AMD_WAVE_SPEC"] = before
    score, best, fresh = d.calculate_score(), d.best_scores(), d.fresh_score()
    reps = []
    for r in range(spec["replicas"]):
        hist, cur = (ctypes.c_int64 * (spec["la"] * 4))(), ctypes.c_int32(-1)
        assert L.sf_debug_late_acceptance(d._h, r, hist, spec["la"], ctypes.byref(cur)) == 0
        reps.append(dict(score=[int(x) for x in score[r]], best=[int(x) for x in best[r]], fresh=[int(x) for x in fresh[r]], lists=d.working_lists(0, r),
                         best_lists=d.working_lists(0, r, best=True), history=[int(x) for x in hist], cursor=cur.value, stats=d.stats(r)))
    res = dict(mode=d.wave_layout()[0], said=said, replicas=reps)
    d.close()
    return res


def _child_run(runs, env):
    """runs = [(spec, knob)] one after another in ONE fresh child process under `env`; a result per run."""
    e = {k: v for k, v in os.environ.items() if k not in MODE_ENVS}
    e.update(env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(runs)], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


_RUNS = {}


def _mode_runs(mode):
    """Every run of one of the modes that need a child, made once and shared: {(case, knob): result}.  Launch mode 6 runs every case once (the
    run-time unit is not offered there); the other modes run EVERY_MODE, under both switches where the mode has a run-time unit (launch mode 4)."""
    if mode not in _RUNS:
        knobs = ("0", "1") if mode == "wpe5" else ("0",)
        runs = [(c, k) for c in (ALL if mode == "node_global" else EVERY_MODE) for k in knobs]
        _RUNS[mode] = dict(zip(runs, _child_run([(ALL[c], k) for c, k in runs], MODES[mode][0])))
    return _RUNS[mode]


# ---- the oracle's run ----------------------------------------------------------------------------------------------------------------
def _oracle_model(spec, r):
    sfo = _SFO["sfo"]
    p = _problem(_pkey(spec))
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=tuple(spec["weights"]))
    assert spec["k"][0] == spec["k"][1]
    o.configure(la_size=spec["la"], limit=spec["limit"], leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=spec["k"][0], random_seed=spec["seed"] + r)
    o.phase_start()
    return o


@functools.lru_cache(maxsize=None)
def _oracle_run(spec_json, r):
    """Replica r through the launches, one step at a time: the state at the end, the best lists as they were when the best score last improved."""
    spec = json.loads(spec_json)
    o = _oracle_model(spec, r)
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    for i, n in enumerate(spec["launches"]):
        at_start = o.stats()["moves_generated"]
        for _ in range(n):
            o.steps(1)
            b = o.best_score()
            if (b != best).any():
                best, best_lists = b.copy(), o.get_lists(0)
            if spec["budget"] and spec["budget"][0] == i and o.stats()["moves_generated"] - at_start >= spec["budget"][1]:
                break
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists, stats=o.stats())


@functools.lru_cache(maxsize=None)
def _oracle_trace(spec_json, r, steps):
    """The first `steps` steps of replica r, traced: per step the leaf of the first pull (0 change, 1 swap; None: no pull), and per leaf the
    number of consumed candidates of each source in the order the sources were scanned."""
    spec = json.loads(spec_json)
    o = _oracle_model(spec, r)
    out = []
    for _ in range(steps):
        moves = o.step_traced()[0]
        per_leaf = ([], [])
        last = [None, None]
        for m in moves:
            leaf = {2: 0, 3: 1}[int(m["kind"])]
            src = (int(m["a"]), int(m["a_pos"]))
            if src != last[leaf]:
                per_leaf[leaf].append(0)
                last[leaf] = src
            per_leaf[leaf][-1] += 1
        out.append(dict(first=None if not len(moves) else {2: 0, 3: 1}[int(moves[0]["kind"])], counts=per_leaf, pulls=len(moves)))
    return out


def _trace(case, r, steps=3):
    return _oracle_trace(json.dumps(CASES[case]), r, steps)


def _check_oracle(spec, got):
    pad = [0] * (spec["levels"] - 2)  # (the padded level: nothing feeds it)
    for r, g in enumerate(got["replicas"]):
        w = _oracle_run(json.dumps(spec), r)
        assert g["score"] == w["score"] + pad, r
        assert g["fresh"] == w["score"] + pad, r  # fresh equals incremental
        assert g["best"] == w["best"] + pad, r
        assert g["lists"] == w["lists"], r
        assert g["best_lists"] == w["best_lists"], r
        for k in ORACLE_WORDS:
            assert g["stats"][k] == w["stats"][k], (r, k)


def _check_reference(got, ref):
    """Every word of every replica against the same solve in launch mode 6: scores, lists, best snapshot, every LateAcceptance slot, the
    history cursor, every sf_stats word."""
    assert ref["mode"] == 6
    for r, (g, w) in enumerate(zip(got["replicas"], ref["replicas"])):
        for word in w:
            assert g[word] == w[word], (r, word)


# ---- what the cases rest on, on the oracle's trace -------------------------------------------------------------------------------------------
def test_premises_on_the_oracle_trace():
    K = 20
    # the round holds: every source a step consumes completely emitted max_nearby (a leaf's last source is cut by the step's end)
    for case in ("holds_limit8", "holds_limit256", "cut_lane0", "cut_lane63", "cut_among_rejections"):
        for r in range(CASES[case]["replicas"]):
            for st in _trace(case, r):
                assert all(c % K == 0 for leaf in st["counts"] for c in leaf[:-1]), (case, r, st)
    # both values of the union's first leaf
    firsts = {st["first"] for r in range(CASES["holds_limit256"]["replicas"]) for st in _trace("holds_limit256", r, 6)}
    assert firsts == {0, 1}, firsts
    # 12 nodes on 3 lists: no source has 20 destinations, the exit comes at the first pass; the steps scan every source
    for r in range(CASES["exit_first_pass"]["replicas"]):
        for st in _trace("exit_first_pass", r):
            assert st["counts"][0][0] % K and st["pulls"] < 12 * 2 * K, st  # (the change leaf's first source already: 13 destinations)
    # 40 nodes on 4 lists: the first sources of both leaves emit 20, later ones fewer (the exit is late), every source is scanned
    late = 0
    for r in range(CASES["exit_late"]["replicas"]):
        for st in _trace("exit_late", r):
            c0, c1 = st["counts"]
            assert any(c % K for c in c0[:-1]) or any(c % K for c in c1[:-1]), st
            late += c0[0] % K == 0 and c1[0] % K == 0
    assert late > 0
    # max_nearby 1: every source emits one candidate, the sources run out with `total` candidates per leaf pending
    # (with 1, 2 or 3 elements most neighbours are unassigned: at most one candidate per source, fewer sources than a batch)
    for case, total in (("runs_out_1", 1), ("runs_out_2", 2), ("runs_out_3", 3), ("runs_out_31", 31)):
        for st in _trace(case, 0):
            assert st["pulls"] <= 2 * total, (case, st)
    assert all(31 < st["pulls"] for st in _trace("runs_out_31", 0))
    assert all(st["pulls"] == 0 for st in _trace("all_lists_empty", 0))


# ---- the default instantiation (launch mode 5), ahead-of-time and run-time unit ---------------------------------------------------------------
@pytest.mark.parametrize("knob", ["0", "1"], ids=["aot", "specialised"])
@pytest.mark.parametrize("case", list(ALL))
def test_lockstep_round(case, knob):
    spec = ALL[case]
    got = _gpu_run(spec, knob)
    assert got["mode"] == 5, got["mode"]
    # the launches under =1 really ran the specialised kernel; those under =0 the ahead-of-time one, by the switch
    assert all(s == ([SPECIALISED, 0] if knob == "1" else [AOT, R_KNOB]) for s in got["said"]), got["said"]
    if case in CASES:
        _check_oracle(spec, got)
    _check_reference(got, _mode_runs("node_global")[(case, "0")])


def test_launch_mode_6_equals_the_oracle():
    """The reference itself: the general loop alone, every case with an oracle."""
    for case, spec in CASES.items():
        _check_oracle(spec, _mode_runs("node_global")[(case, "0")])


# ---- the other instantiations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["no_compact", "wpe4", "wpe5"])
def test_every_instantiation(mode):
    """EVERY_MODE's cases under each mode's switches, one child per mode: launch modes 2, 2 and 4 -- the last under both values of
    SF_AMD_WAVE_SPEC, the others ahead of time (launch mode 2 has no run-time unit: the switch set to 1 changes nothing there)."""
    for (case, knob), got in _mode_runs(mode).items():
        assert got["mode"] == MODES[mode][1], (case, got["mode"])
        if mode == "wpe5":
            assert all(s == ([SPECIALISED, 0] if knob == "1" else [AOT, R_KNOB]) for s in got["said"]), (case, knob, got["said"])
        _check_oracle(ALL[case], got)
        _check_reference(got, _mode_runs("node_global")[(case, "0")])


def test_compact_slice_at_four_waves():
    """Launch mode 3 (the COMPACT slice compiled for 4 waves per SIMD) is taken only by a model too large for 16 wide slices per CU: 1500
    customers on 100 lists, three short launches, under both values of the switch."""
    spec = _spec(_key(1500, 100), launches=(3, 2, 3), la=3, replicas=4)
    a, b = _child_run([(spec, "0"), (spec, "1")], {"SF_AMD_WAVE_WPE": "4"})
    for got, knob in ((a, "0"), (b, "1")):
        assert got["mode"] == 3
        assert all(s == ([SPECIALISED, 0] if knob == "1" else [AOT, R_KNOB]) for s in got["said"]), got["said"]
        _check_oracle(spec, got)
    for r, (g, w) in enumerate(zip(b["replicas"], a["replicas"])):
        for word in w:
            assert g[word] == w[word], (r, word)


if __name__ == "__main__":  # the child: its runs one after another, their results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps([_gpu_run(spec, knob) for spec, knob in json.loads(sys.argv[1])]))
