"""GPU parity tests of the two leg candidates of the wave engine's run-time unit at the smallest shapes that reach every arm of
the replay batch's leg table (eval_generated_small): SF_SPEC_SYM_ROWS addresses two legs by their source-side row, which is the same word only
in a symmetric matrix; SF_SPEC_LEG_REAIM aims the gathers a lane discards at an address the lane fetches anyway.

Every case is a fused solve of three launches of a few steps with 4 replicas.  It runs under SF_AMD_WAVE_SPEC = 0 (the ahead-of-time kernel)
and = 1 with SF_AMD_WAVE_SPEC_EXTRAS unset (the default), = the earlier candidates alone, plus each new bit alone, plus both; sf_debug_wave_spec must name the kernel
that ran and sf_debug_wave_spec_legs the matrix fact and the leg candidates compiled in.  Every replica's working, fresh and best score,
working and best lists and the oracle's seven counters must equal the CPU oracle's bit for bit; every LateAcceptance slot, the history cursor
and every sf_stats word must equal the same solve in launch mode 6 (SF_AMD_NODE_GLOBAL=1, which has no run-time unit; read once per process,
so that solve runs in a fresh child process -- this file run as a script -- one child for all models).

What a case rests on -- which arms of the leg table its first steps price, that a consumed candidate uses the asymmetric leg -- is asserted
on the oracle's trace first."""
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
AOT, SPECIALISED, R_KNOB, R_MODE = 0, 1, 1, 2
X_DEFAULT = 11 | 32 | 64 | 256  # the candidates a launch compiles in when nothing is said (those its facts do not allow are dropped)
X_SYM_ROWS, X_LEG_REAIM = 512, 1024
NEVER = 1 << 20  # an AcceptedCount limit no step reaches: every step scans every source
UNREACHABLE = int(np.iinfo(np.int64).max)
LAUNCHES, LA, REPLICAS, SEED = (5, 4, 6), 400, 4, 5
# (SF_AMD_WAVE_SPEC, SF_AMD_WAVE_SPEC_EXTRAS)
VARIANTS = {"aot": ("0", None), "default": ("1", None), "neither": ("1", X_DEFAULT), "sym_rows": ("1", X_DEFAULT | X_SYM_ROWS), "leg_reaim": ("1", X_DEFAULT | X_LEG_REAIM),
            "both": ("1", X_DEFAULT | X_SYM_ROWS | X_LEG_REAIM)}

_SFO = {}


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    _SFO["sfo"] = oracle
    yield


# ---- models -------------------------------------------------------------------------------------------------------------------------------------
# name: customers, vehicles, start lists' lengths (None: round robin), AcceptedCount limit, the capacity constraint exists, matrix entries set
# after the symmetric matrix is made (as (from, to, value) on the start routes: ("r", list, position) names a node)
MODELS = {
    # 100 nodes on 5 lists: every source has 20 destinations; changes within a list in both directions and to inner and end slots of other
    # lists, the three kinds of swap, sources and destinations at both ends of their lists
    "symmetric": dict(customers=100, vehicles=5, lengths=None, limit=256, capacity=True, entries=[]),
    # 12 nodes on 4 lists of 1, 0, 6 and 5: changes out of a one-element list, an empty list beside them; every step scans every source.  (The
    # table's arm for a change INTO an empty list is never reached by a generated candidate: the nearby meter of a destination in an empty
    # list is not finite -- meters.rs:10-28 -- so the selector never emits one.  The premise test asserts exactly that.)
    "short_lists": dict(customers=12, vehicles=4, lengths=(1, 0, 6, 5), limit=NEVER, capacity=True, entries=[]),
    # 40 nodes on 4 lists without a capacity constraint: no demand word is read
    "no_capacity": dict(customers=40, vehicles=4, lengths=None, limit=256, capacity=False, entries=[]),
    # 30 nodes on 3 lists, one pair of route neighbours whose two directions differ: the source-side rows must not be compiled in
    "one_asymmetric_pair": dict(customers=30, vehicles=3, lengths=None, limit=NEVER, capacity=True, entries=[(("r", 0, 2), ("r", 0, 3), "+5")]),
    # 30 nodes on 3 lists, one leg not finite in both directions: no 32-bit trial arithmetic, so no run-time unit -- the switches change nothing
    "a_leg_not_finite": dict(customers=30, vehicles=3, lengths=None, limit=NEVER, capacity=True,
                             entries=[(("r", 0, 1), ("r", 1, 4), UNREACHABLE), (("r", 1, 4), ("r", 0, 1), UNREACHABLE)]),
}
SYMMETRIC_WORDS = {"symmetric": 1, "short_lists": 1, "no_capacity": 1, "one_asymmetric_pair": 0, "a_leg_not_finite": 1}


@functools.lru_cache(maxsize=None)
def _problem(name):
    from solverforge_amd import datasets

    md = MODELS[name]
    p = datasets.make_cvrp(md["customers"], md["vehicles"], 55, seed=3)
    if md["lengths"] is not None:
        assert len(md["lengths"]) == md["vehicles"] and sum(md["lengths"]) <= md["customers"]
        it = iter(range(1, md["customers"] + 1))
        p["routes"] = [[next(it) for _ in range(n)] for n in md["lengths"]]
    mat = p["matrix"].copy()
    assert (mat == mat.T).all()
    node = lambda ref: p["routes"][ref[1]][ref[2]]  # noqa: E731
    for f, t, v in md["entries"]:
        mat[node(f), node(t)] = mat[node(f), node(t)] + int(v) if isinstance(v, str) else v
    p["matrix"] = np.ascontiguousarray(mat)
    return p


def _director(name):
    import solverforge_amd as sfa
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd.models import FACT_CUSTOMERS, FACT_DEMAND, FACT_MATRIX

    md, p = MODELS[name], _problem(name)
    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=REPLICAS)
    d.add_entity_class(0, len(p["routes"]))
    d.add_list_variable(0, p["routes"], element_capacity=len(p["customers"]), element_id_bound=p["matrix"].shape[0])
    d.add_fact_matrix(FACT_MATRIX, p["matrix"])
    d.add_fact_column_i32(FACT_DEMAND, p["demands"])
    d.add_fact_column_u32(FACT_CUSTOMERS, p["customers"])
    d.add_constraint(ConstraintKind.NOT_EXISTS_FLATTENED, 0, fact=FACT_CUSTOMERS, level=0, weight=1)
    if md["capacity"]:
        d.add_constraint(ConstraintKind.ROUTE_CAPACITY, 0, fact=FACT_DEMAND, param=int(p["capacity"]), level=0, weight=1)
    d.add_constraint(ConstraintKind.ROUTE_DISTANCE, 0, fact=FACT_MATRIX, param=int(p["depot"]), level=1, weight=1)
    d.add_selector(SelectorKind.NEARBY_LIST_CHANGE, 0, max_nearby=20, fact_meter=FACT_MATRIX)
    d.add_selector(SelectorKind.NEARBY_LIST_SWAP, 0, max_nearby=20, fact_meter=FACT_MATRIX)
    d.set_engine(2)
    d.configure(sfa.SolverConfig(late_acceptance_size=LA, accepted_count_limit=md["limit"], random_seed=SEED))
    d.calculate_score()
    d.phase_start()
    return d


# ---- the library's run (in this process or in a child) ------------------------------------------------------------------------------------------
def _gpu_run(name, knob, extras):
    """The solve with every launch under SF_AMD_WAVE_SPEC = knob and SF_AMD_WAVE_SPEC_EXTRAS = extras (None: unset): the launch mode, what
    sf_debug_wave_spec and sf_debug_wave_spec_legs said after each launch, and the state left behind in every replica."""
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    for f in ("sf_debug_wave_spec", "sf_debug_wave_spec_legs", "sf_debug_late_acceptance"):
        getattr(L, f).restype = ctypes.c_int32
    d = _director(name)
    env = {"SF_AMD_WAVE_SPEC": knob, "SF_AMD_WAVE_SPEC_EXTRAS": None if extras is None else str(extras)}
    before = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    said = []
    try:
        for n in LAUNCHES:
            d.solve_steps(n)
            out, legs = (ctypes.c_int32 * 26)(), (ctypes.c_int32 * 2)()
            assert L.sf_debug_wave_spec(d._h, out, len(out)) == 0 and L.sf_debug_wave_spec_legs(d._h, legs, 2) == 0
            said.append([out[0], out[1], legs[0], legs[1], out[4 + 21] & (X_SYM_ROWS | X_LEG_REAIM)])
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    score, best, fresh = d.calculate_score(), d.best_scores(), d.fresh_score()
    reps = []
    for r in range(REPLICAS):
        hist, cur = (ctypes.c_int64 * (LA * 4))(), ctypes.c_int32(-1)
        assert L.sf_debug_late_acceptance(d._h, r, hist, LA, ctypes.byref(cur)) == 0
        reps.append(dict(score=[int(x) for x in score[r]], best=[int(x) for x in best[r]], fresh=[int(x) for x in fresh[r]], lists=d.working_lists(0, r),
                         best_lists=d.working_lists(0, r, best=True), history=[int(x) for x in hist], cursor=cur.value, stats=d.stats(r)))
    res = dict(mode=d.wave_layout()[0], said=said, replicas=reps)
    d.close()
    return res


_REFERENCE = {}


def _reference(name):
    """Every model once in launch mode 6, in ONE fresh child process, shared."""
    if not _REFERENCE:
        e = {k: v for k, v in os.environ.items() if k not in ("SF_AMD_NO_COMPACT", "SF_AMD_WAVE_WPE", "SF_AMD_WAVE_SPEC", "SF_AMD_WAVE_SPEC_EXTRAS")}
        e["SF_AMD_NODE_GLOBAL"] = "1"
        res = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(list(MODELS))], env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        _REFERENCE.update(zip(MODELS, json.loads(res.stdout.strip().splitlines()[-1])))
    return _REFERENCE[name]


# ---- the oracle's run ---------------------------------------------------------------------------------------------------------------------------
def _oracle_model(name, r):
    sfo = _SFO["sfo"]
    md, p = MODELS[name], _problem(name)
    o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=(1, 1 if md["capacity"] else 0, 1))
    o.configure(la_size=LA, limit=md["limit"], leaves=sfo.LEAF_NEARBY_LIST_CHANGE | sfo.LEAF_NEARBY_LIST_SWAP, max_nearby=20, random_seed=SEED + r)
    o.phase_start()
    return o


@functools.lru_cache(maxsize=None)
def _oracle_run(name, r):
    """Replica r through the launches, one step at a time: the state at the end, the best lists as they were when the best score last improved."""
    o = _oracle_model(name, r)
    best, best_lists = o.best_score().copy(), o.get_lists(0)
    for _ in range(sum(LAUNCHES)):
        o.steps(1)
        b = o.best_score()
        if (b != best).any():
            best, best_lists = b.copy(), o.get_lists(0)
    return dict(score=[int(x) for x in o.score()[:2]], best=[int(x) for x in best[:2]], lists=o.get_lists(0), best_lists=best_lists, stats=o.stats())


def _arms(lists, depot, m):
    """The arms of the leg table one consumed candidate reaches, and the (from, to) legs whose words enter its delta (the table of
    eval_list_move_small; a leg a lane fetches and discards is not among them)."""
    chg, a, i, b, j = int(m["kind"]) == 2, int(m["a"]), int(m["a_pos"]), int(m["b"]), int(m["b_pos"])
    A, B = lists[a], lists[b]
    la, lb, intra = len(A), len(B), a == b
    at = lambda lst, k: lst[k] if 0 <= k < len(lst) else depot  # noqa: E731
    x, pa, na = A[i], at(A, i - 1), at(A, i + 1)
    vq, pb, nb = at(B, j), at(B, j - 1), at(B, j + 1)
    adj = not chg and intra and j == i + 1
    arms = {"source_first" if i == 0 else "source_inner", "source_last" if i == la - 1 else "source_inner"}
    if chg:
        arms.add("change_forward" if intra and j > i else "change_backward" if intra else "change_empty" if lb == 0 else "change_end" if j == lb else "change_inner")
        arms.add("destination_first" if j == 0 else "destination_last" if j == lb else "destination_inner")
        if la == 1:
            arms.add("change_out_of_single")
        plus = ([] if la == 1 else [(pa, na)]) + [(pb, x), (x, vq)]
        minus = [(pa, x), (x, na)] + ([] if (not intra and lb == 0) else [(pb, vq)])
    else:
        assert j < lb and not (intra and j <= i)
        arms.add("swap_adjacent" if adj else "swap_intra" if intra else "swap_cross")
        arms.add("destination_first" if j == 0 else "destination_last" if j == lb - 1 else "destination_inner")
        if adj:
            plus, minus = [(pa, vq), (vq, x), (x, nb)], [(pa, x), (x, vq), (vq, nb)]
        else:
            plus, minus = [(pa, vq), (vq, na), (pb, x), (x, nb)], [(pa, x), (x, na), (pb, vq), (vq, nb)]
    return arms, plus + minus


@functools.lru_cache(maxsize=None)
def _oracle_premises(name, steps=4):
    """Over the first `steps` steps of every replica: the arms the consumed candidates reach, and the legs they price."""
    depot = int(_problem(name)["depot"])
    arms, legs = set(), set()
    for r in range(REPLICAS):
        o = _oracle_model(name, r)
        for _ in range(steps):
            lists = o.get_lists(0)
            for m in o.step_traced()[0]:
                a, l = _arms(lists, depot, m)
                arms |= a
                legs |= set(l)
    return arms, legs


def test_premises_on_the_oracle_trace():
    every_swap = {"swap_adjacent", "swap_intra", "swap_cross"}
    ends = {"source_first", "source_last", "source_inner", "destination_first", "destination_last", "destination_inner"}
    arms, _ = _oracle_premises("symmetric")
    assert {"change_forward", "change_backward", "change_inner", "change_end"} | every_swap | ends <= arms, arms
    arms, _ = _oracle_premises("short_lists")
    assert {"change_out_of_single", "change_end", "change_inner"} | every_swap <= arms, arms
    assert [] in _problem("short_lists")["routes"] and "change_empty" not in arms  # (an empty list is no nearby destination: see MODELS)
    arms, _ = _oracle_premises("no_capacity")
    assert {"change_inner", "swap_cross", "swap_intra"} <= arms, arms
    # the asymmetric pair: a consumed candidate prices the leg in each direction, and the two words differ
    p = _problem("one_asymmetric_pair")
    u, v = p["routes"][0][2], p["routes"][0][3]
    assert p["matrix"][u, v] == p["matrix"][v, u] + 5
    _, legs = _oracle_premises("one_asymmetric_pair")
    assert (u, v) in legs and (v, u) in legs
    # the not-finite leg is priced too
    p = _problem("a_leg_not_finite")
    u, v = p["routes"][0][1], p["routes"][1][4]
    assert p["matrix"][u, v] == UNREACHABLE == p["matrix"][v, u]
    _, legs = _oracle_premises("a_leg_not_finite")
    assert (u, v) in legs or (v, u) in legs


def test_the_fact_of_each_model():
    """What sf_initialize will find, through the same reduction on the host (sf_debug_mat_sym)."""
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_mat_sym.restype = ctypes.c_int32
    for name, want in SYMMETRIC_WORDS.items():
        m, out = _problem(name)["matrix"], (ctypes.c_int32 * 1)(-1)
        assert L.sf_debug_mat_sym(m.ctypes.data_as(ctypes.c_void_p), m.shape[0], out, 1) == 0 and out[0] == want, name


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def _check_oracle(name, got):
    for r, g in enumerate(got["replicas"]):
        w = _oracle_run(name, r)
        assert g["score"] == w["score"], r
        assert g["fresh"] == w["score"], r  # fresh equals incremental
        assert g["best"] == w["best"], r
        assert g["lists"] == w["lists"], r
        assert g["best_lists"] == w["best_lists"], r
        for k in ORACLE_WORDS:
            assert g["stats"][k] == w["stats"][k], (r, k)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(MODELS))
def test_leg_candidates(name, variant):
    knob, extras = VARIANTS[variant]
    got = _gpu_run(name, knob, extras)
    ref = _reference(name)
    small = name != "a_leg_not_finite"
    if small:
        assert got["mode"] == 5 and ref["mode"] == 6, (got["mode"], ref["mode"])
    else:
        assert got["mode"] not in (3, 4, 5, 6), got["mode"]
    # which kernel ran, the matrix fact in its key, and the leg candidates compiled in: one the fact does not allow is dropped
    sym = SYMMETRIC_WORDS[name]
    asked = X_SYM_ROWS if extras is None else extras  # (nothing said: the default, the source-side rows)
    want_bits = (asked & X_LEG_REAIM) | ((asked & X_SYM_ROWS) if sym else 0)
    for state, reason, mat_sym, leg_bits, index_bits in got["said"]:
        assert [state, reason] == ([AOT, R_KNOB] if knob == "0" else [SPECIALISED, 0] if small else [AOT, R_MODE]), got["said"]
        assert mat_sym == sym and leg_bits == index_bits, got["said"]
        if state == SPECIALISED:
            assert leg_bits == want_bits, (got["said"], want_bits)
    _check_oracle(name, got)
    for r, (g, w) in enumerate(zip(got["replicas"], ref["replicas"])):
        for word in w:
            assert g[word] == w[word], (r, word)


def test_launch_mode_6_equals_the_oracle():
    """The reference itself."""
    for name in MODELS:
        _check_oracle(name, _reference(name))


if __name__ == "__main__":  # the child: every model once, the results as one JSON line
    sys.path.insert(0, ROOT)
    print(json.dumps([_gpu_run(name, "0", None) for name in json.loads(sys.argv[1])]))
