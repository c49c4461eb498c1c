"""The local-search step protocol (acceptor -> forager -> step_ended; forager.rs:143-420, improving.rs, step.rs:216-221,
diversified_late_acceptance.rs:161-170, scope_progress.rs:89-107) at every place that runs it: the block engine, the wave engine's
general replay, the generic engine, the fused scalar engine and the host-driven provider step (sf_step_decide_cursor).

What the other suites leave thin: the forager's tie-break carried across 64-candidate chunks with `random_ties` on AND off (the
reservoir pick of forager.rs:143-148 against "the first of the equals stays"), in fused launches split in two.  The models are built to
tie: a CVRP on an integer grid with Manhattan distances, a sparse graph colouring.  Scores, best scores, the working state and the seven
counters are compared with the oracle per replica; the oracle's own runs with and without random ties must end in different states, or
the comparison would say nothing about the tie-break."""
import numpy as np
import pytest

from test_gpu_anneal import _graph
from test_gpu_foragers import COUNTERS

pytestmark = pytest.mark.gpu

DLA, TOLERANCE, LA_SIZE = 4, 0.02, 5
# (acceptor, forager, accepted_count_limit; 0 = None).  AcceptedCount(70): a step consumes more than one 64-candidate chunk.
CASES = [(0, 2, 0), (1, 0, 70), (1, 3, 0), (1, 4, 0), (DLA, 2, 1)]
TIES = [True, False]
R = 3
ORDER_RANDOM, ORDER_SHUFFLED = 3, 4

# engine, leaves, selection order.  The block engine does not carry DiversifiedLateAcceptance (refused on the host:
# test_gpu_diversified.test_validation), so it has no such case.  LateAcceptance + AcceptedCount + SelectionOrder::Random takes the wave
# engine to its FAST kernels: the SMALL ones have a replay of their own (delta keys), the other one runs the general replay compiled for
# that policy and has no case here.  Shuffled keeps every case of the wave engine on the general kernel.
LIST_SITES = {
    "block": (1, ("nearby_change", "nearby_swap"), ORDER_RANDOM),
    "wave": (2, ("nearby_change", "nearby_swap"), ORDER_SHUFFLED),
    "generic": (0, ("nearby_change", "nearby_swap", "list_reverse"), ORDER_RANDOM),
}
LEAF_BITS = {"nearby_change": 16, "nearby_swap": 32, "list_reverse": 64}
LIST_PARAMS = [(site,) + case for site in LIST_SITES for case in CASES if not (site == "block" and case[0] == DLA)]
LIST_STEPS, LIST_SEED = 40, 13
GRAPH_N, GRAPH_STEPS, GRAPH_SEED = 60, 40, 5
DECIDE_STEPS = 12

_memo = {}


def _grid_cvrp():
    """36 customers on a 6 x 6 integer grid (the depot on a grid point of its own), Manhattan distances, 4 vehicles."""
    from solverforge_amd import datasets

    pts = [(3, 7)] + [(x, y) for y in range(6) for x in range(6)]
    xs, ys = np.array([p[0] for p in pts], dtype=np.int64), np.array([p[1] for p in pts], dtype=np.int64)
    dim = len(pts)
    demands = (datasets.stream(41, dim) % np.uint64(5)).astype(np.int32) + 1
    demands[0] = 0
    routes = [[] for _ in range(4)]
    for c in range(1, dim):
        routes[(c * 7) % 4].append(c)
    return {"capacity": 30, "depot": 0, "demands": demands,
            "matrix": np.ascontiguousarray(np.abs(xs[:, None] - xs[None, :]) + np.abs(ys[:, None] - ys[None, :])),
            "customers": np.arange(1, dim, dtype=np.uint32), "routes": routes}


def _configure_oracle(o, case, ties, order, bits, seed):
    acceptor, forager, limit = case
    o.configure(acceptor=1 if acceptor == DLA else acceptor, la_size=LA_SIZE, forager=forager, limit=limit, random_ties=ties,
                selection_order=order, leaves=bits, random_seed=seed)
    if acceptor == DLA:
        o.configure_diversified(LA_SIZE, TOLERANCE)
    o.phase_start()


def _configure_gpu(d, case, ties, order, seed):
    import solverforge_amd as sfa

    acceptor, forager, limit = case
    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=LA_SIZE, forager=forager, accepted_count_limit=limit,
                                 random_ties=ties, selection_order=order, random_seed=seed))
    if acceptor == DLA:
        d.configure_diversified(TOLERANCE)
    d.calculate_score()
    d.phase_start()


def _list_oracle(oracle, site, case, ties):
    """Per replica: (score, best score, lists, stats) of the oracle's run -- computed once per configuration."""
    key = ("list", site, case, ties)
    if key not in _memo:
        _, leaves, order = LIST_SITES[site]
        p = _grid_cvrp()
        out = []
        for r in range(R):
            o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
            _configure_oracle(o, case, ties, order, sum(LEAF_BITS[x] for x in leaves), LIST_SEED + r)
            o.steps(LIST_STEPS)
            out.append((o.score()[:2].copy(), o.best_score()[:2].copy(), o.get_lists(0), o.stats()))
        _memo[key] = out
    return _memo[key]


def _graph_oracle(oracle, case, ties):
    key = ("graph", case, ties)
    if key not in _memo:
        g = _graph(n=GRAPH_N, e=150, k=4, seed=11)
        out = []
        for r in range(R):
            o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
            _configure_oracle(o, case, ties, ORDER_RANDOM, oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, GRAPH_SEED + r)
            o.steps(GRAPH_STEPS)
            out.append((o.score()[:2].copy(), o.best_score()[:2].copy(), o.get_vars(0, 0).copy(), o.stats()))
        _memo[key] = out
    return _memo[key]


def _decide_graph(oracle):
    """The colouring after a hill climb: improving candidates are rare from here on, so the improving foragers too consume whole stores
    and fall back on the best of the accepted candidates, ties included."""
    if "decide_graph" not in _memo:
        g = _graph(n=GRAPH_N, e=150, k=4, seed=11)
        o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
        _configure_oracle(o, (0, 2, 0), True, ORDER_RANDOM, 3, GRAPH_SEED)
        o.steps(12)
        g["colors"] = o.get_vars(0, 0).astype(np.int64).copy()
        _memo["decide_graph"] = g
    return _memo["decide_graph"]


def _decide_candidates(g, step):
    """The provider's store of one step: every (node, colour) change, rotated by the step -- five chunks, no-ops (not doable) included."""
    n, k = g["n"], g["n_colors"]
    c = [[(v, col)] for v in range(n) for col in range(k)]
    s = (step * 37) % len(c)
    return c[s:] + c[:s]


def _decide_oracle(oracle, case, ties):
    """Per replica: the per-step (scores, flags, pick) and the final (score, best score, values, stats)."""
    key = ("decide", case, ties)
    if key not in _memo:
        g = _decide_graph(oracle)
        out = []
        for r in range(2):
            o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
            _configure_oracle(o, case, ties, ORDER_RANDOM, 3, GRAPH_SEED + r)
            steps = []
            for step in range(DECIDE_STEPS):
                sc, fl, sel = o.step_cursor(_decide_candidates(g, step))
                steps.append((sc[:, :2].copy(), fl.copy(), sel))
            out.append((steps, o.score()[:2].copy(), o.best_score()[:2].copy(), o.get_vars(0, 0).copy(), o.stats()))
        _memo[key] = out
    return _memo[key]


def _differ(a, b, state):
    """Some replica's working state (element `state` of its record) differs between two oracle runs."""
    return any(not np.array_equal(np.asarray(x[state], dtype=object), np.asarray(y[state], dtype=object)) for x, y in zip(a, b))


def _same_counters(gst, ost, r):
    for k in COUNTERS:
        assert gst[k] == ost[k], (r, k, gst[k], ost[k])


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("site,acceptor,forager,limit", LIST_PARAMS)
def test_list_engines(oracle, site, acceptor, forager, limit, ties):
    import solverforge_amd as sfa

    case = (acceptor, forager, limit)
    # the tie-break decides this model's search: the oracle alone ends elsewhere without it
    assert _differ(_list_oracle(oracle, site, case, True), _list_oracle(oracle, site, case, False), 2)
    engine, leaves, order = LIST_SITES[site]
    d = sfa.build_cvrp(_grid_cvrp(), n_replicas=R, leaves=leaves)
    if engine:
        d.set_engine(engine)
    _configure_gpu(d, case, ties, order, LIST_SEED)
    d.solve_steps(LIST_STEPS // 2)
    d.solve_steps(LIST_STEPS - LIST_STEPS // 2)
    scores, best = d.calculate_score(), d.best_scores()
    for r, (osc, obest, olists, ost) in enumerate(_list_oracle(oracle, site, case, ties)):
        assert (scores[r] == osc).all(), r
        assert (best[r] == obest).all(), r
        assert d.working_lists(0, r) == olists, r
        _same_counters(d.stats(r), ost, r)
    assert (d.fresh_score() == scores).all()


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("acceptor,forager,limit", CASES)
def test_scalar_engine(oracle, acceptor, forager, limit, ties):
    import solverforge_amd as sfa

    case = (acceptor, forager, limit)
    assert _differ(_graph_oracle(oracle, case, True), _graph_oracle(oracle, case, False), 2)
    d = sfa.build_graph_coloring(_graph(n=GRAPH_N, e=150, k=4, seed=11), n_replicas=R)
    _configure_gpu(d, case, ties, ORDER_RANDOM, GRAPH_SEED)
    d.solve_steps(GRAPH_STEPS // 2)
    d.solve_steps(GRAPH_STEPS - GRAPH_STEPS // 2)
    scores, best = d.calculate_score(), d.best_scores()
    for r, (osc, obest, ovals, ost) in enumerate(_graph_oracle(oracle, case, ties)):
        assert (scores[r] == osc).all(), r
        assert (best[r] == obest).all(), r
        assert (d.working_values(0, 0, replica=r) == ovals).all(), r
        _same_counters(d.stats(r), ost, r)
    assert (d.fresh_score() == scores).all()


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("acceptor,forager,limit", CASES)
def test_provider_step(oracle, acceptor, forager, limit, ties):
    """k_scalar_step_decide: the candidates come from the host, in pull order; one launch per step and replica."""
    import solverforge_amd as sfa

    case = (acceptor, forager, limit)
    on, off = _decide_oracle(oracle, case, True), _decide_oracle(oracle, case, False)
    assert _differ(on, off, 3)
    g = _decide_graph(oracle)
    d = sfa.build_graph_coloring(g, n_replicas=2)
    _configure_gpu(d, case, ties, ORDER_RANDOM, GRAPH_SEED)
    want = _decide_oracle(oracle, case, ties)
    for step in range(DECIDE_STEPS):
        cands = _decide_candidates(g, step)
        for r in range(2):
            gs, gf, gsel = d.step_decide_cursor(cands, replica=r)
            os_, of, osel = want[r][0][step]
            assert len(gf) == len(of) and (gf == of).all(), (step, r)
            assert (gs == os_).all(), (step, r)
            assert gsel == osel, (step, r)
    scores, best = d.calculate_score(), d.best_scores()
    for r, (_, osc, obest, ovals, ost) in enumerate(want):
        assert (scores[r] == osc).all(), r
        assert (best[r] == obest).all(), r
        assert (d.working_values(0, 0, replica=r) == ovals).all(), r
        _same_counters(d.stats(r), ost, r)
    assert (d.fresh_score() == scores).all()
