"""GPU parity tests of the wave engine's run-time specialisation: the kernel compiled in process for a context's constants
against the ahead-of-time kernel of the same launch mode.

Every case runs the same fused solve of three launches in one process under three settings of SF_AMD_WAVE_SPEC (read at every launch):
0, 0, 0 -- the ahead-of-time kernel; 1, 1, 1 -- the specialised one; 0, 1, 0 -- each kernel reads the state the other wrote back.  After
every launch sf_debug_wave_spec must name the kernel that ran (state 1 = specialised, key = the model's constants).  The three runs must
leave the same state behind in every replica: working and best scores, working and best lists, every LateAcceptance slot and the history
cursor (sf_debug_late_acceptance), every sf_stats word; replica 0 must equal the CPU oracle.

Shapes are small ones at which baked constants can go wrong: V in {2, 3, 64, 65, 128, 129} (the order tables' chunk edges, the use_cm gate),
dim in {5, 32, 33, 65} (a neighbour row shorter than a half, than a chunk, one entry more), max_nearby in {1, 20, 32, 33, 64} (the ring-size
switch at 32 / 33), a list longer than the position field of the 16-bit node table (the saturation count), launch modes 3, 4 and 5
(SF_AMD_WAVE_WPE is read once per process: those run in a child, this file as a script), and the four-level unit through a three-level
CVRP.  A dozen distinct keys in all; each compile's milliseconds are printed."""
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
AOT, SPECIALISED, FELL_BACK = 0, 1, 2
R_KNOB, R_NO_SOURCES = 1, 11
KEY_WORDS = 18  # WaveSpecKey: levels, wpe, V, dim, n_cap, k0, k1, extras and the ten words of the candidates (zero while their bit is off)
LAUNCHES = (6, 5, 7)
ORDERS = ("000", "111", "010")
LONG_LENGTHS = [1] + [0] * 3 + [2] + [0] * 70 + [63, 64, 65, 520]  # 79 lists: 7 route bits, 9 position bits -- 520 > pmax = 511


def _spec(customers, vehicles, max_nearby=20, levels=2, capacity=55, lengths=None, replicas=3, la=3, seed=5):
    """la = 3: over launches of 6, 5 and 7 steps the history cursor wraps inside every launch and ends each on a different slot."""
    return dict(customers=customers, vehicles=vehicles, max_nearby=max_nearby, levels=levels, capacity=capacity, lengths=lengths, replicas=replicas, la=la, seed=seed)


def _problem(spec):
    from solverforge_amd import datasets

    p = datasets.make_cvrp(spec["customers"], spec["vehicles"], spec["capacity"], seed=3)
    if spec["lengths"] is not None:
        assert len(spec["lengths"]) == spec["vehicles"] and sum(spec["lengths"]) == spec["customers"]
        it = iter(range(1, spec["customers"] + 1))
        p["routes"] = [[next(it) for _ in range(n)] for n in spec["lengths"]]
    return p


def _director(spec, p):
    import solverforge_amd as sfa

    if spec["levels"] == 2:
        d = sfa.build_cvrp(p, n_replicas=spec["replicas"], max_nearby=spec["max_nearby"])
    else:  # the same CVRP under three score levels, the third fed by nothing: plan_wave_launch takes the four-level unit for it
        from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
        from solverforge_amd.models import FACT_CUSTOMERS, FACT_DEMAND, FACT_MATRIX

        d = GpuScoreDirector(score_levels=spec["levels"], hard_levels=1, n_replicas=spec["replicas"])
        d.add_entity_class(0, len(p["routes"]))
        d.add_list_variable(0, p["routes"], element_capacity=len(p["customers"]), element_id_bound=p["matrix"].shape[0])
        d.add_fact_matrix(FACT_MATRIX, p["matrix"])
        d.add_fact_column_i32(FACT_DEMAND, p["demands"])
        d.add_fact_column_u32(FACT_CUSTOMERS, p["customers"])
        d.add_constraint(ConstraintKind.NOT_EXISTS_FLATTENED, 0, fact=FACT_CUSTOMERS, level=0, weight=1)
        d.add_constraint(ConstraintKind.ROUTE_CAPACITY, 0, fact=FACT_DEMAND, param=int(p["capacity"]), level=0, weight=1)
        d.add_constraint(ConstraintKind.ROUTE_DISTANCE, 0, fact=FACT_MATRIX, param=int(p["depot"]), level=1, weight=1)
        d.add_selector(SelectorKind.NEARBY_LIST_CHANGE, 0, max_nearby=spec["max_nearby"], fact_meter=FACT_MATRIX)
        d.add_selector(SelectorKind.NEARBY_LIST_SWAP, 0, max_nearby=spec["max_nearby"], fact_meter=FACT_MATRIX)
    d.set_engine(2)
    d.configure(sfa.SolverConfig(late_acceptance_size=spec["la"], random_seed=spec["seed"]))
    d.calculate_score()
    d.phase_start()
    return d


def _spec_state(d=None):
    """sf_debug_wave_spec: state and reason of the context's last wave launch, compiles of the process, the last compile's ms, the key."""
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    out = (ctypes.c_int32 * (4 + KEY_WORDS))()
    L.sf_debug_wave_spec.restype = ctypes.c_int32
    assert L.sf_debug_wave_spec(d._h if d is not None else None, out, len(out)) == 0
    return dict(state=out[0], reason=out[1], compiles=out[2], ms=out[3], key=list(out[4:]))


def _history(d, r, la):
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_late_acceptance.restype = ctypes.c_int32
    out, cur = (ctypes.c_int64 * (la * 4))(), ctypes.c_int32(-1)
    assert L.sf_debug_late_acceptance(d._h, r, out, la, ctypes.byref(cur)) == 0
    return [int(x) for x in out], cur.value


def _snapshot(d, spec):
    score, best, fresh = d.calculate_score(), d.best_scores(), d.fresh_score()
    reps = []
    for r in range(spec["replicas"]):
        hist, cursor = _history(d, r, spec["la"])
        reps.append(dict(score=[int(x) for x in score[r]], best=[int(x) for x in best[r]], fresh=[int(x) for x in fresh[r]], lists=d.working_lists(0, r),
                         best_lists=d.working_lists(0, r, best=True), history=hist, cursor=cursor, stats=d.stats(r)))
    return reps


def _solve(spec, order, p=None, d=None):
    """The three launches under SF_AMD_WAVE_SPEC = order[i]; what sf_debug_wave_spec said after each, and the state left behind."""
    p = _problem(spec) if p is None else p
    d = _director(spec, p) if d is None else d
    before = os.environ.get("SF_AMD_WAVE_SPEC")
    said = []
    try:
        for n, knob in zip(LAUNCHES, order):
            os.environ["SF_AMD_WAVE_SPEC"] = knob
            d.solve_steps(n)
            said.append(_spec_state(d))
    finally:
        if before is None:
            os.environ.pop("SF_AMD_WAVE_SPEC", None)
        else:
            os.environ["SF_AMD_WAVE_SPEC"] = before
    out = dict(mode=d.wave_layout()[0], renumbered=d.wave_layout()[1], said=said, replicas=_snapshot(d, spec))
    d.close()
    return out


def _case(spec):
    """The solve under the three orders, in this process."""
    p = _problem(spec)
    return {order: _solve(spec, order, p) for order in ORDERS}


X_DEFAULT = 1 | 2 | 8  # SF_WSPEC_X_DEFAULT: capacity / weights / depot / level words, the history's size, the node numbering's presence


def _expected_key(spec, mode, renumbered, extras=X_DEFAULT):
    """The key of a launch: the instantiation, the five constants, the candidates compiled in.  The depot (word 11) is the model's -- 0 -- under
    the caller's numbering and whatever the internal numbering made of it otherwise: None = not compared."""
    key = [2 if spec["levels"] <= 2 else 4, {3: 4, 4: 5, 5: 6}[mode], spec["vehicles"], spec["customers"] + 1, spec["customers"], spec["max_nearby"], spec["max_nearby"], extras]
    key += [spec["capacity"], 1, 1, None if renumbered else 0, 0, 1] if extras & 1 else [0] * 6
    key += [spec["la"] if extras & 2 else 0, 256 if extras & 4 else 0, int(renumbered) if extras & 8 else 0, 0]
    return key


def _key_is(got, want):
    return len(got) == len(want) == KEY_WORDS and all(w is None or g == w for g, w in zip(got, want))


_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


@functools.lru_cache(maxsize=None)
def _oracle(spec_json):
    spec = json.loads(spec_json)
    sfo = _SFO["sfo"]
    p = _problem(spec)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=spec["la"], limit=256, leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=spec["max_nearby"], random_seed=spec["seed"])
    o.phase_start()
    o.steps(sum(LAUNCHES))
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in o.best_score()[:2]], lists=o.get_lists(0), stats=o.stats())


def _check(spec, runs, mode):
    for order, run in runs.items():
        assert run["mode"] == mode, (order, run["mode"])
        key = _expected_key(spec, mode, run["renumbered"])
        for knob, s in zip(order, run["said"]):
            assert _key_is(s["key"], key), (order, s, key)
            # the launch under =1 really was the specialised kernel; the one under =0 the ahead-of-time one, by the switch
            assert (s["state"], s["reason"]) == ((SPECIALISED, 0) if knob == "1" else (AOT, R_KNOB)), (order, s)
    ms = runs["111"]["said"][0]["ms"]
    print("key", key, "compile ms", ms)
    ref = runs["000"]["replicas"]
    for order in ("111", "010"):
        for r, (a, b) in enumerate(zip(ref, runs[order]["replicas"])):
            for word in a:
                assert a[word] == b[word], (order, r, word)  # lists, scores, best snapshot, every history slot and its cursor, every sf_stats word
    w = _oracle(json.dumps(spec))
    pad = [0] * (spec["levels"] - 2)
    g = ref[0]
    assert g["score"] == w["score"] + pad and g["fresh"] == w["score"] + pad and g["best"] == w["best"] + pad and g["lists"] == w["lists"]
    for k in ORACLE_WORDS:
        assert g["stats"][k] == w["stats"][k], k


# ---- launch mode 5, the two-level unit: the shapes ------------------------------------------------------------------------------------------------
SHAPES = {
    "V2_dim5_k1": _spec(4, 2, max_nearby=1),          # a row of five entries: shorter than a half of the paired pass; V - 1 = 1
    "V3_dim32_k20": _spec(31, 3),                     # a row of exactly one half
    "V3_dim33_k32": _spec(32, 3, max_nearby=32),      # ... one entry more; the 64-entry ring at its largest max_nearby
    "V64_dim65_k33": _spec(64, 64, max_nearby=33),    # one chunk of lists, a row one entry past a chunk, the 128-entry ring at its smallest max_nearby
    "V65_k64": _spec(133, 65, max_nearby=64, capacity=20),
    "V128_k20": _spec(259, 128, capacity=20),         # use_cm's last size
    "V129_k20": _spec(261, 129, capacity=20),         # ... and the first past it: the scalar permutation parameters
    "long_list": _spec(sum(LONG_LENGTHS), len(LONG_LENGTHS), capacity=2000, lengths=LONG_LENGTHS, replicas=2),  # nsat > 0: the saturation scan
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    spec = SHAPES[name]
    _check(spec, _case(spec), 5)


# ---- the four-level unit; launch modes 3 and 4 -------------------------------------------------------------------------------------------------
def test_four_level_unit():
    spec = _spec(40, 4, levels=3)
    _check(spec, _case(spec), 5)


def _child(payload, env):
    e = {k: v for k, v in os.environ.items() if k not in ("SF_AMD_WAVE_WPE", "SF_AMD_WAVE_SPEC", "SF_AMD_CSRC")}
    e.update(env)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(payload)], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("wpe,mode,spec", [("5", 4, _spec(40, 4)), ("4", 3, _spec(1500, 100, replicas=2))], ids=["mode4", "mode3"])
def test_other_modes(wpe, mode, spec):
    """SF_AMD_WAVE_WPE=5: launch mode 4.  =4 and a model too large for 16 wide slices per CU (1500 customers on 100 lists): launch mode 3."""
    _check(spec, _child(dict(what="case", spec=spec), {"SF_AMD_WAVE_WPE": wpe}), mode)


# ---- the candidate constants (SF_AMD_WAVE_SPEC_EXTRAS: diagnostics, read at every launch) ----------------------------------------------------------
def test_every_candidate_compiled_in(levels=2):
    """All five candidates at once -- capacity, weights, depot and level words; the history's size; the AcceptedCount limit; the node numbering's
    presence; explicit seeds' absence -- leave the same state behind as the ahead-of-time kernel."""
    spec = _spec(40, 4, levels=levels)
    p = _problem(spec)
    ref = _solve(spec, "000", p)
    os.environ["SF_AMD_WAVE_SPEC_EXTRAS"] = "31"
    try:
        got = _solve(spec, "111", p)
    finally:
        del os.environ["SF_AMD_WAVE_SPEC_EXTRAS"]
    for s in got["said"]:
        assert s["state"] == SPECIALISED and _key_is(s["key"], _expected_key(spec, 5, got["renumbered"], extras=31)), s
    assert got["replicas"] == ref["replicas"]


# ---- the cache ---------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_alive_and_an_equal_one():
    """Two contexts with different constants alive at once, their launches interleaved; then a second context with the constants of the
    first: it compiles nothing."""
    sa, sb = SHAPES["V3_dim32_k20"], SHAPES["V3_dim33_k32"]  # (keys the shape cases compile too: a dozen distinct keys in the whole file)
    pa, pb = _problem(sa), _problem(sb)
    ref_a, ref_b = _solve(sa, "000", pa), _solve(sb, "000", pb)
    da, db = _director(sa, pa), _director(sb, pb)
    os.environ["SF_AMD_WAVE_SPEC"] = "1"
    try:
        for n in LAUNCHES:
            da.solve_steps(n)
            db.solve_steps(n)
            assert _spec_state(da)["state"] == SPECIALISED and _spec_state(db)["state"] == SPECIALISED
        assert _key_is(_spec_state(da)["key"], _expected_key(sa, 5, da.wave_layout()[1])) and _key_is(_spec_state(db)["key"], _expected_key(sb, 5, db.wave_layout()[1]))
        assert _snapshot(da, sa) == ref_a["replicas"] and _snapshot(db, sb) == ref_b["replicas"]
        compiles = _spec_state()["compiles"]
        assert compiles >= 2
        dc = _director(sa, pa)
        for n in LAUNCHES:
            dc.solve_steps(n)
            assert _spec_state(dc)["state"] == SPECIALISED
        assert _spec_state()["compiles"] == compiles
        assert _snapshot(dc, sa) == ref_a["replicas"]
        dc.close()
    finally:
        del os.environ["SF_AMD_WAVE_SPEC"]
        da.close()
        db.close()


def test_no_sources_falls_back(tmp_path):
    """SF_AMD_CSRC at an empty directory: nothing raised, the launch ran the ahead-of-time kernel (state "fell back": no sources), same results."""
    spec = _spec(40, 4)
    got = _child(dict(what="solve", spec=spec, order="111"), {"SF_AMD_CSRC": str(tmp_path)})
    assert [(s["state"], s["reason"]) for s in got["said"]] == [(FELL_BACK, R_NO_SOURCES)] * 3 and got["said"][-1]["compiles"] == 0
    assert got["replicas"] == _solve(spec, "000")["replicas"]


if __name__ == "__main__":  # the child: one case or one solve, its result as one JSON line
    sys.path.insert(0, ROOT)
    job = json.loads(sys.argv[1])
    print(json.dumps(_case(job["spec"]) if job["what"] == "case" else _solve(job["spec"], job["order"])))
