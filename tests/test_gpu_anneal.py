"""GPU parity tests (through the C ABI): SimulatedAnnealing acceptor on every search engine vs the
CPU oracle (phase/localsearch/acceptor/simulated_annealing.rs).  Candidate order, trial scores,
accept flags, applied moves, counters and the f64 temperatures must agree exactly.

The tie rule: the Boltzmann test uses the device exp(), which may differ from glibc's by one ulp, so a draw with
|u - probability| <= 4 * spacing(probability) is undecidable, and only at such a draw might a flag differ.  The scripted
sequences of tests/anneal_chunk_cases.py are proven free of such draws on the oracle alone (tests/test_anneal_chunk_cases.py)
and compared flag by flag on the device (tests/test_gpu_anneal_chunks.py); the runs here are whole searches, where one
differing flag changes every later candidate and fails the comparison at that step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SA = 3


def _t(moves):
    return np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1)


def _graph(n=120, e=500, k=5, seed=11):
    from solverforge_amd import datasets

    g = datasets.make_graph(n, e, k, seed=seed)
    r = datasets.stream(seed + 99, n)
    g["colors"] = (r % np.uint64(k + 1)).astype(np.int64) - 1
    return g


def _configure(d, o, oracle, bits, forager, limit, seed, anneal, levels=2, hard_levels=1, max_nearby=20):
    import solverforge_amd as sfa

    o.configure(acceptor=1, la_size=5, forager=forager, limit=limit, leaves=bits, random_seed=seed, max_nearby=max_nearby)
    o.configure_annealing(levels=levels, hard_levels=hard_levels, seed=seed, **anneal)
    d.configure(sfa.SolverConfig(acceptor=SA, forager=forager, accepted_count_limit=limit, random_seed=seed))
    kw = dict(anneal)
    d.configure_annealing(mode=kw.pop("mode", 2), temperatures=kw.pop("temperatures", ()),
                          decay_rate=kw.pop("decay_rate", 0.999985),
                          hill_climbing_temperature=kw.pop("hill_climbing_temperature", 1.0e-9),
                          never_accept_hard_regression=kw.pop("never_accept_hard", False),
                          calibration_sample_size=kw.pop("sample_size", 128),
                          target_acceptance_probability=kw.pop("target_probability", 0.80),
                          fallback_temperature=kw.pop("fallback_temperature", 1.0), seed=seed)
    assert not kw


def _compare_state(d, o, levels=2):
    gt, gc = d.annealing_state(0)
    ot, _, oc = o.annealing_state()
    assert gc == bool(oc)
    assert (gt.view(np.uint64) == ot[:levels].view(np.uint64)).all(), (gt, ot)


def _traced(d, o, steps, levels=2, worse_levels=None, states=None):
    """worse_levels: a list that receives the first differing level of every accepted worsening candidate; states: a list that
    receives the oracle's (temperatures, calibrating) after every step."""
    d.calculate_score()
    d.phase_start()
    o.phase_start()
    accepted_worse = 0
    for step in range(steps):
        last = o.score()[:levels].copy()
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 17)
        om, os_, of, oap, omv = o.step_traced()
        assert len(gm) == len(om), step
        assert (_t(gm) == _t(om)).all(), step
        assert (gs == os_[:, :levels]).all(), step
        assert (gf == of).all(), step
        assert gap == oap, step
        if gap:
            assert tuple(gmv[k] for k in gmv.dtype.names) == tuple(omv[k] for k in omv.dtype.names), step
        for sc, fl in zip(os_[:, :levels], of):
            if fl & 2 and tuple(sc) < tuple(last):
                accepted_worse += 1
                if worse_levels is not None:
                    worse_levels.append(int(np.flatnonzero(sc != last)[0]))
        _compare_state(d, o, levels)
        if states is not None:
            ot, _, oc = o.annealing_state()
            states.append((ot[:levels].copy(), bool(oc)))
    assert (d.calculate_score()[0] == o.score()[:levels]).all()
    assert (d.best_scores()[0] == o.best_score()[:levels]).all()
    gst, ost = d.stats(0), o.stats()
    for k in ["step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied",
              "score_calculations", "moves_not_doable"]:
        assert gst[k] == ost[k], k
    return accepted_worse


ANNEAL_CASES = [
    # the scalar-only default policy: auto-calibrated, AcceptedCount(1) (policy.rs:56-77)
    (dict(mode=2), 0, 1),
    (dict(mode=2, sample_size=24, target_probability=0.5), 0, 7),   # calibration completes inside a chunk
    (dict(mode=0, temperatures=(3.0,), decay_rate=0.97), 0, 4),
    (dict(mode=1, temperatures=(0.5, 40.0), decay_rate=0.9, hill_climbing_temperature=2.0), 1, 1),
    (dict(mode=1, temperatures=(50.0, 50.0), never_accept_hard=True), 0, 16),
    (dict(mode=2, sample_size=5, fallback_temperature=2.5), 2, 1),  # BestScore forager: whole neighbourhood
]


@pytest.mark.parametrize("anneal,forager,limit", ANNEAL_CASES)
def test_graph_annealing_traced_steps(oracle, anneal, forager, limit):
    import solverforge_amd as sfa

    g = _graph()
    d = sfa.build_graph_coloring(g, n_replicas=1)
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    _configure(d, o, oracle, oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, forager, limit, 17, anneal)
    worse = _traced(d, o, 12 if forager == 2 else 160)
    if anneal.get("mode") == 0 or anneal.get("sample_size", 128) < 30:
        assert worse > 0  # the Boltzmann branch really ran


def test_graph_annealing_fused_matches_oracle(oracle):
    """Fused multi-step launches (no trace): final values, scores, counters, temperatures, per replica seed."""
    import solverforge_amd as sfa

    g = _graph(n=200, e=900, k=6, seed=5)
    R = 3
    d = sfa.build_graph_coloring(g, n_replicas=R)
    d.configure(sfa.SolverConfig(acceptor=SA, forager=0, accepted_count_limit=1, random_seed=40))
    d.configure_annealing(mode=2, calibration_sample_size=40, seed=40)
    d.calculate_score()
    d.phase_start()
    d.solve_steps(250)
    d.solve_steps(150)
    for r in (0, 2):
        o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
        o.configure(acceptor=1, forager=0, limit=1, leaves=oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP,
                    random_seed=40 + r)
        o.configure_annealing(mode=2, sample_size=40, seed=40 + r)
        o.phase_start()
        o.steps(400)
        assert (d.working_values(0, 0, replica=r) == o.get_vars(0, 0)).all()
        assert (d.calculate_score()[r] == o.score()[:2]).all()
        assert (d.best_scores()[r] == o.best_score()[:2]).all()
        gt, gc = d.annealing_state(r)
        ot, _, oc = o.annealing_state()
        assert gc == bool(oc) and (gt.view(np.uint64) == ot[:2].view(np.uint64)).all()
        gst, ost = d.stats(r), o.stats()
        for k in ["step_count", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations"]:
            assert gst[k] == ost[k], k


@pytest.mark.parametrize("engine", [1, 2])  # block, wave
@pytest.mark.parametrize("anneal,limit", [(dict(mode=2, sample_size=30), 8), (dict(mode=0, temperatures=(25.0,), decay_rate=0.99), 3)])
def test_cvrp_annealing_traced_steps(oracle, engine, anneal, limit):
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_cvrp(60, 6, 45, seed=9)
    d = sfa.build_cvrp(p, n_replicas=1, max_nearby=10)
    d.set_engine(engine)
    o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    _configure(d, o, oracle, oracle.LEAF_NEARBY_LIST_CHANGE | oracle.LEAF_NEARBY_LIST_SWAP, 0, limit, 23, anneal, max_nearby=10)
    assert _traced(d, o, 60) > 0


def test_generic_engine_annealing_traced_steps(oracle):
    """Union with plain leaves -> the N-leaf engine."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_cvrp(40, 5, 40, seed=4)
    leaves = ("nearby_change", "list_swap", "list_reverse")
    d = sfa.build_cvrp(p, n_replicas=1, max_nearby=8, leaves=leaves)
    o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    bits = oracle.LEAF_NEARBY_LIST_CHANGE | oracle.LEAF_LIST_SWAP | oracle.LEAF_LIST_REVERSE
    _configure(d, o, oracle, bits, 0, 5, 31, dict(mode=2, sample_size=20), max_nearby=8)
    assert _traced(d, o, 50) > 0


def test_large_magnitude_annealing_scalar_engine(oracle):
    """58-bit costs: the calibration's level-1 total passes 2^64 (the high word of the 128-bit sum, its conversion to f64), and
    delta / T runs on 58-bit deltas against a temperature near 2^60.  Scalar engine, calibrated over 512 samples."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    n, k = 16, 8
    r = datasets.stream(3, n + n * k)
    values = (r[:n] % np.uint64(k)).astype(np.int64)
    cost = ((r[n:] >> np.uint64(6)) | np.uint64(1)).astype(np.int64).reshape(n, k)
    assert int(cost.max()).bit_length() == 58
    d = sfa.build_assignment(values, cost, k, ex_level=-1, cost_weight=1)
    o = oracle.Model.assignment(values, cost, k, ex_level=-1, cost_weight=1)
    _configure(d, o, oracle, oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, 0, 1, 3, dict(mode=2, sample_size=512))
    states = []
    worse = _traced(d, o, 60, states=states)
    done = [i for i, (_, calibrating) in enumerate(states) if not calibrating]
    assert done and 0 < done[0] < 59  # steps on both sides of the completion were traced
    t_done = states[done[0]][0]  # after that step's own cooling: a little below the installed temperature
    assert t_done[1] * -np.log(0.8) * 512 > 2 ** 64  # mean = T * -ln(p): the level-1 total had a non-zero high word
    assert worse > 0
    d.solve_steps(340)  # a fused window behind the traced steps
    o.steps(340)
    assert (d.working_values(0, 0, replica=0) == o.get_vars(0, 0)).all()
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.best_scores()[0] == o.best_score()[:2]).all()
    _compare_state(d, o)
    gst, ost = d.stats(0), o.stats()
    for key in ["step_count", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations"]:
        assert gst[key] == ost[key], key
    model, gen = d.arith_flags()
    assert model["scalar_value_bytes"] != 0 and gen is None, (model, gen)  # the scalar engine ran, the generic one never


@pytest.mark.parametrize("anneal,limit", [
    (dict(mode=2, sample_size=40), 8),
    (dict(mode=1, temperatures=(0.7, 3.0, 25.0), decay_rate=0.99), 4),
    (dict(mode=1, temperatures=(50.0, 50.0, 50.0), never_accept_hard=True), 16),
])
def test_three_level_annealing_generic_engine(oracle, anneal, limit):
    """The four-level build of the acceptor inside an engine: three score levels, two of them hard, three temperatures cooling.
    Every worsening candidate this model accepts differs first at level index 2 (no hard-level draw happens on it even at
    T = 6); hard-level draws of the four-level build are the harness's job (tests/test_gpu_anneal_chunks.py)."""
    import solverforge_amd as sfa

    from test_gpu_large_launch import _JobShop

    p = _JobShop()._problem()  # the 12 x 5 mixed job shop: BendableScore<2, 1>, four leaves
    d = sfa.build_jobshop(p, n_replicas=1, bendable=True)
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=True)
    bits = oracle.LEAF_LIST_CHANGE | oracle.LEAF_LIST_SWAP | oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    _configure(d, o, oracle, bits, 0, limit, 13, anneal, levels=3, hard_levels=2)
    levels = []
    assert _traced(d, o, 80, levels=3, worse_levels=levels) > 0
    assert set(levels) == {2}
    _, gen = d.arith_flags()
    assert gen is not None and gen["levels"] == 4, gen


def test_three_level_annealing_scalar_engine(oracle):
    """The scalar engine's four-level build: an assignment on three levels (unassigned / cost / rows in use), costs in 0..2 so
    that candidates differ first at level 2 as well."""
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd import datasets
    from solverforge_amd.models import FACT_COLUMN, FACT_MATRIX

    n, k = 12, 8
    r = datasets.stream(21, n + n * k + k)
    values = (r[:n] % np.uint64(k + 1)).astype(np.int64) - 1
    cost = (r[n:n + n * k] % np.uint64(3)).astype(np.int64).reshape(n, k)
    row_w = (r[n + n * k:] % np.uint64(9)).astype(np.int64) + 1
    d = GpuScoreDirector(score_levels=3, hard_levels=1, n_replicas=1)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, k, True, values)
    d.add_fact_matrix(FACT_MATRIX, cost)
    d.add_fact_column_i32(FACT_COLUMN, row_w.astype(np.int32))
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    d.add_constraint(ConstraintKind.VALUE_COST, 0, fact=FACT_MATRIX, level=1, weight=1)
    d.add_constraint(ConstraintKind.EXISTS_VALUE, 0, fact=FACT_COLUMN, param=1, level=2, weight=3)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    o = oracle.Model.assignment(values, cost, k, row_w=row_w, ex_mode=1, ex_level=2, ex_weight=3)
    _configure(d, o, oracle, oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, 0, 4, 19, dict(mode=2, sample_size=30), levels=3, hard_levels=1)
    levels = []
    assert _traced(d, o, 100, levels=3, worse_levels=levels) > 0
    assert {1, 2} <= set(levels)
    model, gen = d.arith_flags()
    assert model["scalar_value_bytes"] != 0 and gen is None, (model, gen)


def test_annealing_parameter_validation():
    """assert_simulated_annealing_parameters (simulated_annealing.rs:305-336) -> SF_ERR_INVALID."""
    import solverforge_amd as sfa

    d = sfa.build_nqueens([-1] * 8)
    for bad in [dict(decay_rate=0.0), dict(decay_rate=1.5), dict(hill_climbing_temperature=-1.0),
                dict(mode=1, temperatures=(1.0, float("inf"))), dict(calibration_sample_size=0),
                dict(target_acceptance_probability=1.0), dict(fallback_temperature=float("nan"))]:
        with pytest.raises(sfa.SolverForgeError):
            d.configure_annealing(**bad)
    d.configure_annealing()
