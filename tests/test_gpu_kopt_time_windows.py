"""GPU parity tests (through the C ABI): the complete route_hooks::feasible of the stock CVRP domain (capacity + time windows,
crates/solverforge-cvrp/src/helpers.rs:109-119, 168-218) on the device -- feasible_mode 2 of sf_construct_list_k_opt, sf_list_set_time_windows,
sf_list_routes_feasible -- against the oracle (oracle/sfo_clarke_wright.hpp list_k_opt with the hook of sfo_capi.cpp, pinned to the reference's own
test by tests/test_oracle_cvrp_time_windows.py).  Every comparison is bit-exact: the lists of EVERY replica, committed scores, fresh_score and
the deltas of the solver counters.  The inputs of the parity sweep satisfy the condition tests/test_cvrptw_dataset.py asserts on the CPU (the
oracle's mode-2 run accepts something and differs from its mode-0 run); it is asserted again here on the runs that are compared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 10**6  # capacity out of the way: the windows alone decide
I64_MAX = int(np.iinfo(np.int64).max)
UNREACHABLE = I64_MAX
COUNTERS = ["step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations"]


def _family(slack):
    return [
        ("plain-60/6", dict(n_customers=60, n_vehicles=6, capacity=BIG, seed=3, slack=slack, tw_seed=1)),
        ("ragged-130/9", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2)),
        ("one-route-130", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2, one_route=True)),
        ("one-route-130-lo=arrival", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2, one_route=True, lo_slack=0)),
    ]


# the same list as tests/test_cvrptw_dataset.py::PARITY_CASES
PARITY_CASES = [c for s in (300, 1000, 3000) for c in _family(s)] + [
    ("cvrp-1000/100-cap55", dict(n_customers=1000, n_vehicles=100, capacity=55, seed=0, slack=s, tw_seed=3)) for s in (1000, 3000)]
IDS = [f"{name}-slack{kw['slack']}" for name, kw in PARITY_CASES]


def _oracle_model(oracle, p, windows=True):
    m = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    if windows:
        lo, hi = p["time_windows"]
        m.set_time_windows(lo, hi, p["service"], p["travel"], p.get("departure", 0))
    return m


def _without_windows(p):
    return {k: v for k, v in p.items() if k not in ("time_windows", "service", "travel", "departure")}


def _run_and_compare(d, oracles, mode, max_sweeps):
    """One k-opt run of the device against one oracle model per replica (the same model for all when the replicas are equal).
    Returns the oracle's stats per replica."""
    R = d.n_replicas
    d.construct_list_k_opt(0, 3, mode, max_sweeps)  # k != 2: scored no-op (also allocates the counters)
    g0 = [d.stats(r) for r in range(R)]
    o0 = [o.stats() for o in oracles]
    sc = d.construct_list_k_opt(0, 2, mode, max_sweeps)
    sts = [o.construct_list_k_opt(2, mode, max_sweeps) for o in oracles]
    fresh = d.fresh_score()
    for r in range(R):
        o = oracles[r % len(oracles)]
        assert d.working_lists(0, r) == o.get_lists(0), r
        assert (sc[r] == o.score()[:2]).all(), r
        assert (fresh[r] == o.score()[:2]).all(), r
        gst, ost = d.stats(r), o.stats()
        for k in COUNTERS:
            assert gst[k] - g0[r][k] == ost[k] - o0[r % len(oracles)][k], (r, k)
    return sts


def _reference_plan():  # list_cvrp_k_opt_time_window/domain/plan.rs:46-88
    m = np.full((5, 5), 100, dtype=np.int64)
    np.fill_diagonal(m, 0)
    for (a, b, v) in [(0, 1, 1), (1, 3, 50), (3, 2, 1), (2, 4, 50), (4, 0, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)]:
        m[a, b] = v
    t = np.zeros((5, 5), dtype=np.int64)
    t[1, 2] = 10
    t[2, 3] = 10
    return dict(capacity=100, depot=0, demands=np.array([0, 1, 1, 1, 1], dtype=np.int32), matrix=m, customers=np.arange(1, 5, dtype=np.uint32),
                routes=[[1, 3, 2, 4]], time_windows=(np.zeros(5, np.int64), np.array([100, 100, 100, 5, 100], dtype=np.int64)),
                service=np.zeros(5, np.int64), travel=t, departure=0)


def test_reference_case_the_window_breaking_reversal_is_refused(oracle):
    """crates/solverforge/tests/list_cvrp_k_opt_time_window.rs:9-41: the reversal that would shorten [1, 3, 2, 4] to [1, 2, 3, 4] reaches
    customer 3 after its window has closed."""
    import solverforge_amd as sfa

    p = _reference_plan()
    d = sfa.build_cvrp(p, n_replicas=3)
    o = _oracle_model(oracle, p)
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    assert d.routes_feasible(0, 2).tolist() == [[1]] * 3
    sts = _run_and_compare(d, [o], 2, 1000)
    assert int(sts[0][0]) > 0 and int(sts[0][1]) == 0
    for r in range(3):
        assert d.working_lists(0, r) == [[1, 3, 2, 4]]
        assert d.stats(r)["moves_accepted"] == 0
    d1 = sfa.build_cvrp(p, n_replicas=3)
    o1 = _oracle_model(oracle, p)
    d1.calculate_score()
    _run_and_compare(d1, [o1], 1, 1000)
    for r in range(3):
        assert d1.working_lists(0, r) == [[1, 2, 3, 4]]
    assert d1.routes_feasible(0, 2).tolist() == [[0]] * 3 and d1.routes_feasible(0, 1).tolist() == [[1]] * 3
    assert not o1.route_feasible([1, 2, 3, 4]) and o1.route_feasible([1, 3, 2, 4])


@pytest.mark.parametrize("path", ["gated", "walk"])
@pytest.mark.parametrize("max_sweeps", [1000, 3])
@pytest.mark.parametrize("name,kw", PARITY_CASES, ids=IDS)
def test_mode_2_matches_oracle(oracle, name, kw, max_sweeps, path):
    """path "gated": what the host range check picks (the composed fold on all of these); "walk": the checked lane-serial walk forced."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(**kw)
    d = sfa.build_cvrp(p, n_replicas=3)
    o = _oracle_model(oracle, p)
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    assert d.time_window_path(0, force_walk=(path == "walk")) == ("walk" if path == "walk" else "composed")
    before = o.get_lists(0)
    start_flags = d.routes_feasible(0, 2)
    for r in range(3):
        assert start_flags[r].tolist() == [int(o.route_feasible(rt)) for rt in before]
    sts = _run_and_compare(d, [o], 2, max_sweeps)
    assert d.time_window_path(0, last_ran=True) == ("walk" if path == "walk" else "composed")  # as the 2-opt kernel itself reports it
    o_free = _oracle_model(oracle, p)
    o_free.construct_list_k_opt(2, 0, max_sweeps)
    assert int(sts[0][1]) >= 1 and o.get_lists(0) != o_free.get_lists(0)  # the condition on the inputs (tests/test_cvrptw_dataset.py)
    end_flags = d.routes_feasible(0, 2)
    after = o.get_lists(0)
    for r in range(3):
        assert end_flags[r].tolist() == [int(o.route_feasible(rt)) for rt in after]
    for e, rt in enumerate(before):  # the hook at work: a route that was feasible stays feasible, an infeasible one is left alone
        assert end_flags[0][e] == start_flags[0][e] and (start_flags[0][e] or after[e] == rt)


@pytest.mark.parametrize("n,v,seed,cap", [(130, 9, 21, BIG), (150, 12, 6, 70)])
def test_replicas_that_differ(oracle, n, v, seed, cap):
    """Four replicas diverge over 10 fused local-search steps (replica r of a context seeded s is the oracle seeded s + r), then mode 2:
    each replica against an oracle model that took the same steps.  Local search ignores the windows, so it is kept short: every
    replica's oracle run still accepts reversals and differs from the mode-0 run of the same state."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    R, STEPS = 4, 10
    p = datasets.make_cvrptw(n_customers=n, n_vehicles=v, capacity=cap, seed=seed, slack=3000, tw_seed=5)
    bits = oracle.LEAF_NEARBY_LIST_CHANGE | oracle.LEAF_NEARBY_LIST_SWAP
    d = sfa.build_cvrp(p, n_replicas=R)
    d.configure(sfa.SolverConfig(random_seed=5))
    d.calculate_score()
    d.phase_start()
    d.solve_steps(STEPS)
    oracles, free = [], []
    for r in range(R):
        for keep in (oracles, free):
            o = _oracle_model(oracle, p)
            o.configure(leaves=bits, random_seed=5 + r)
            o.phase_start()
            o.steps(STEPS)
            keep.append(o)
        assert d.working_lists(0, r) == oracles[r].get_lists(0), r
    assert len({str(o.get_lists(0)) for o in oracles}) == R  # four different solutions
    flags = d.routes_feasible(0, 2)
    for r in range(R):
        assert flags[r].tolist() == [int(oracles[r].route_feasible(rt)) for rt in oracles[r].get_lists(0)], r
    sts = _run_and_compare(d, oracles, 2, 1000)
    for r in range(R):
        free[r].construct_list_k_opt(2, 0, 1000)
        assert int(sts[r][1]) >= 1 and oracles[r].get_lists(0) != free[r].get_lists(0), r


# ---- the predicate on edge data: sf_list_routes_feasible vs the oracle's route_feasible ------------------------------------------------
def _predicate_problem(rng, n=25, n_routes=7):
    """Random asymmetric distance and travel (travel != distance), disjoint random routes with two empty ones."""
    m = rng.integers(1, 30, (n, n)).astype(np.int64)
    np.fill_diagonal(m, 0)
    perm = rng.permutation(np.arange(1, n)).tolist()
    cuts = sorted(rng.choice(np.arange(1, len(perm)), n_routes - 3, replace=False).tolist())
    routes = [perm[a:b] for a, b in zip([0] + cuts, cuts + [len(perm)])]
    routes = routes[:2] + [[]] + routes[2:] + [[]]
    demands = rng.integers(0, 7, n).astype(np.int32)
    demands[0] = 0
    return dict(capacity=int(rng.integers(12, 30)), depot=0, demands=demands, matrix=m, customers=np.arange(1, n, dtype=np.uint32), routes=routes)


def _check_predicate(oracle, d, p, lo, hi, service, travel, dep, modes=(1, 2), paths=(False, True)):
    o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.set_time_windows(lo, hi, service, travel, dep)
    d.set_time_windows(0, lo, hi, service, travel, dep)
    want2 = [int(o.route_feasible(rt)) for rt in p["routes"]]
    want1 = [int(not rt or sum(int(p["demands"][c]) for c in rt) <= p["capacity"]) for rt in p["routes"]]
    for force in paths:
        d.time_window_path(0, force_walk=force)
        for r in range(d.n_replicas):
            if 2 in modes:
                assert d.routes_feasible(0, 2)[r].tolist() == want2, (force, r)
            if 1 in modes:
                assert d.routes_feasible(0, 1)[r].tolist() == want1, (force, r)
    d.time_window_path(0, force_walk=False)
    return want1, want2


def test_routes_feasible_on_seeded_routes(oracle):
    """Seeded like tests/test_oracle_cvrp_time_windows.py: random travel != distance, asymmetric, departure != 0, about half of the routes
    infeasible, some over capacity; both evaluation paths."""
    import solverforge_amd as sfa

    rng = np.random.default_rng(11)
    seen1, seen2 = set(), set()
    for case in range(12):
        p = _predicate_problem(rng)
        n = len(p["demands"])
        d = sfa.build_cvrp(p, n_replicas=2)
        d.calculate_score()
        for sub in range(5):
            t = rng.integers(0, 12, (n, n)).astype(np.int64)
            if sub == 0:
                t[rng.integers(0, n), rng.integers(0, n)] = UNREACHABLE
            lo = rng.integers(0, 30, n).astype(np.int64)
            hi = lo + rng.integers(20, 120, n)
            service = rng.integers(0, 6, n).astype(np.int64)
            want1, want2 = _check_predicate(oracle, d, p, lo, hi, service, t, int(rng.integers(0, 15)))
            assert d.time_window_path(0) == "composed"
            seen1.update(want1), seen2.update(w2 for w1, w2, rt in zip(want1, want2, p["routes"]) if w1 and rt)
    assert seen1 == {0, 1} and seen2 == {0, 1}  # over-capacity routes, and capacity-feasible routes on both sides of the windows


def _wide(p, rng):
    """Windows every route passes: the edge cases below each break exactly one thing."""
    n = len(p["demands"])
    t = rng.integers(1, 12, (n, n)).astype(np.int64)
    return np.zeros(n, np.int64), np.full(n, 10**6, np.int64), rng.integers(0, 6, n).astype(np.int64), t


EDGES = ["unreachable-leg", "negative-leg", "unreachable-back-leg", "negative-back-leg", "negative-service", "lo>hi", "hi-max-service-max",
         "hi-max", "departure-near-max", "departure-near-max-zero-legs", "lo-min", "unused-legs-only"]


@pytest.mark.parametrize("edge", EDGES)
def test_routes_feasible_on_edge_data(oracle, edge):
    """One irregularity at a time on otherwise wide-open windows (capacity out of the way); the expected verdicts are the oracle's and, where
    the recurrence makes them obvious, stated."""
    import solverforge_amd as sfa

    rng = np.random.default_rng(5)
    p = _predicate_problem(rng)
    p["capacity"] = BIG
    routes = [rt for rt in p["routes"] if rt]
    d = sfa.build_cvrp(p, n_replicas=2)
    d.calculate_score()
    lo, hi, service, t = _wide(p, rng)
    dep = 3
    hit = routes[1]  # the route the irregularity is placed on
    assert len(hit) >= 2 and len(routes) >= 3
    others_ok = True
    if edge == "unreachable-leg":
        t[hit[0], hit[1]] = UNREACHABLE
    elif edge == "negative-leg":
        t[0, hit[0]] = -1
    elif edge == "unreachable-back-leg":
        t[hit[-1], 0] = UNREACHABLE
    elif edge == "negative-back-leg":
        t[hit[-1], 0] = -5
    elif edge == "negative-service":
        service[hit[-1]] = -1
    elif edge == "lo>hi":
        lo[hit[0]], hi[hit[0]] = 500, 499
    elif edge == "hi-max-service-max":  # t + service overflows (tests/test_cvrp_data.py:69-70)
        hi[hit[1]], service[hit[1]] = I64_MAX, I64_MAX
    elif edge == "hi-max":  # a window that never closes: feasible, but outside the range check
        hi[:] = I64_MAX
        hit = None
    elif edge == "departure-near-max":  # the first leg overflows on every route
        dep, hi[:] = I64_MAX - 1, I64_MAX
        hit, others_ok = None, False
    elif edge == "departure-near-max-zero-legs":  # nothing is added: feasible at the very top of i64
        dep, hi[:] = I64_MAX, I64_MAX
        t[:], service[:] = 0, 0
        hit = None
    elif edge == "lo-min":  # a window that opened long ago
        lo[:] = np.iinfo(np.int64).min
        hit = None
    elif edge == "unused-legs-only":  # irregular entries on legs no route uses change nothing
        used = {(a, b) for rt in routes for a, b in zip([0] + rt, rt + [0])}
        for a in range(len(lo)):
            for b in range(len(lo)):
                if (a, b) not in used:
                    t[a, b] = UNREACHABLE if (a + b) % 2 else -7
        hit = None
    _, want2 = _check_predicate(oracle, d, p, lo, hi, service, t, dep, modes=(2,))
    for rt, w in zip(p["routes"], want2):
        assert w == int(not rt or (others_ok and rt != hit)), (edge, rt)
    expect_path = "walk" if edge in ("hi-max-service-max", "hi-max", "departure-near-max", "departure-near-max-zero-legs", "lo-min") else "composed"
    assert d.time_window_path(0) == expect_path


def test_over_capacity_routes_under_modes_1_and_2(oracle):
    import solverforge_amd as sfa

    rng = np.random.default_rng(8)
    p = _predicate_problem(rng)
    loads = [sum(int(p["demands"][c]) for c in rt) for rt in p["routes"]]
    p["capacity"] = sorted(loads)[len(loads) // 2]  # the heavier routes are over capacity, the one at the bound is not
    d = sfa.build_cvrp(p, n_replicas=2)
    d.calculate_score()
    lo, hi, service, t = _wide(p, rng)
    want1, want2 = _check_predicate(oracle, d, p, lo, hi, service, t, 0)
    assert want1 == want2 and set(want1) == {0, 1}
    hi[p["routes"][loads.index(p["capacity"])][-1]] = 0  # a capacity-feasible route now misses a window
    want1b, want2b = _check_predicate(oracle, d, p, lo, hi, service, t, 0)
    assert want1b == want1 and sum(want2b) == sum(want2) - 1


# ---- the host range check: one step inside, one step outside ------------------------------------------------------------------------
def _gate_bound(p, n_cap):
    lo, hi = p["time_windows"]
    t = p["travel"]
    fin = t[(t >= 0) & (t != UNREACHABLE)]
    return abs(int(p["departure"])) + (n_cap + 1) * (int(fin.max()) + max(0, int(p["service"].max()))) + max(int(np.abs(lo).max()), int(np.abs(hi).max()))


@pytest.mark.parametrize("shape", ["unvisited-node", "shifted-times"])
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_range_check_edges(oracle, shape, side):
    """sf_list_set_time_windows admits the composed fold when |departure| + (element_capacity + 1) (max finite travel + max service) +
    max |lo|, |hi| < 2^59.  "unvisited-node": the depot's own `hi` (never read by the recurrence) carries the bound to 2^59 - 1 / 2^59;
    "shifted-times": departure and every window are shifted up together until the bound sits there, so the composed fold works on
    sums near its limit.  Either side equals the oracle in a full mode-2 run and the path that ran is asserted."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(n_customers=60, n_vehicles=6, capacity=BIG, seed=3, slack=1000, tw_seed=1)
    lo, hi = (a.copy() for a in p["time_windows"])
    n_cap, limit = 60, 1 << 59
    target = limit - 1 if side == "inside" else limit
    if shape == "unvisited-node":
        hi[0] = 0
        p["time_windows"] = (lo, hi)
        hi[0] = target - _gate_bound(p, n_cap) + int(np.abs(hi).max())
        assert hi[0] == int(np.abs(hi).max())
    else:
        hi[0] = 0
        p["time_windows"] = (lo, hi)
        room = target - _gate_bound(p, n_cap)  # = 2 K for a shift of K (departure and the largest |hi| both move), up to parity
        k = room // 2
        lo += k
        hi += k
        p["departure"] = k
        hi[0] = int(hi.max()) + (room - 2 * k)
    assert _gate_bound(p, n_cap) == target
    d = sfa.build_cvrp(p, n_replicas=2)
    o = _oracle_model(oracle, p)
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    assert d.time_window_path(0) == ("composed" if side == "inside" else "walk")
    before = o.get_lists(0)
    assert d.routes_feasible(0, 2)[1].tolist() == [int(o.route_feasible(rt)) for rt in before] == [1] * 6
    sts = _run_and_compare(d, [o], 2, 1000)
    o_free = _oracle_model(oracle, p)
    o_free.construct_list_k_opt(2, 0, 1000)
    assert int(sts[0][1]) >= 1 and o.get_lists(0) != o_free.get_lists(0)
    assert d.time_window_path(0) == ("composed" if side == "inside" else "walk")
    assert d.time_window_path(0, last_ran=True) == ("composed" if side == "inside" else "walk")  # as the kernel itself reports it


# ---- validation ------------------------------------------------------------------------------------------------------------------
def test_validation(oracle):
    import solverforge_amd as sfa
    from solverforge_amd import datasets
    from solverforge_amd._lib import ptr

    p = datasets.make_cvrptw(n_customers=60, n_vehicles=6, capacity=BIG, seed=3, slack=1000, tw_seed=1)
    lo, hi = p["time_windows"]
    d = sfa.build_cvrp(_without_windows(p), n_replicas=2)
    d.calculate_score()
    assert d.time_window_path(0) == "none"
    with pytest.raises(sfa.SolverForgeError):
        d.construct_list_k_opt(0, 2, 2)  # mode 2 before the windows are set
    with pytest.raises(sfa.SolverForgeError):
        d.routes_feasible(0, 2)
    assert d.routes_feasible(0, 1).tolist() == [[1] * 6] * 2  # capacity alone needs no windows
    with pytest.raises(sfa.SolverForgeError):
        d.set_time_windows(0, lo[:-1], hi[:-1], p["service"][:-1], p["travel"][:-1, :-1])  # wrong n_nodes
    with pytest.raises(sfa.SolverForgeError):
        d.set_time_windows(1, lo, hi, p["service"], p["travel"])  # not the list class
    L, h = d._L, d._h
    tr = np.ascontiguousarray(p["travel"])
    for missing in range(4):
        args = [ptr(lo), ptr(hi), ptr(p["service"]), ptr(tr)]
        args[missing] = None
        assert L.sf_list_set_time_windows(h, 0, len(lo), *args, 0) != 0  # NULL array
    assert L.sf_list_routes_feasible(h, 0, 1, None) != 0
    assert d.time_window_path(0) == "none"
    # setting the windows twice: the second set wins.  First a set under which nothing is feasible, then the real one
    d.set_time_windows(0, lo, np.full_like(hi, -1), p["service"], p["travel"])
    assert d.routes_feasible(0, 2).tolist() == [[0] * 6] * 2
    d.set_time_windows(0, lo, hi, p["service"], p["travel"], p["departure"])
    assert d.routes_feasible(0, 2).tolist() == [[1] * 6] * 2
    for mode in (3, -1):
        with pytest.raises(sfa.SolverForgeError):
            d.construct_list_k_opt(0, 2, mode)
    for mode in (0, 3):
        with pytest.raises(sfa.SolverForgeError):
            d.routes_feasible(0, mode)
    with pytest.raises(sfa.SolverForgeError):
        d.construct_list_k_opt(0, 2, 2, 0)  # max_sweeps >= 1
    o = _oracle_model(oracle, p)
    _run_and_compare(d, [o], 2, 1000)  # ... and the run under the second set equals the oracle's
    # windows handed over BEFORE sf_initialize with a wrong node count surface at initialize
    d2 = sfa.build_cvrp(_without_windows(p), n_replicas=1)
    big = len(lo) + 3
    d2.set_time_windows(0, np.zeros(big, np.int64), np.zeros(big, np.int64), np.zeros(big, np.int64), np.zeros((big, big), np.int64))
    with pytest.raises(sfa.SolverForgeError):
        d2.calculate_score()


def test_a_precedence_model_is_refused():
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    q = datasets.make_precedence_shop(4, 3, seed=2)
    d = sfa.build_precedence_shop(q)
    d.calculate_score()
    n = len(q["durations"])
    z = np.zeros(n, np.int64)
    d.set_time_windows(0, z, z + 10**6, z, np.zeros((n, n), np.int64))  # the tables themselves are data of the list class: accepted
    with pytest.raises(sfa.SolverForgeError):
        d.construct_list_k_opt(0, 2, 2)


@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_do_not_read_the_windows(oracle, mode):
    """The same model with and without windows set: modes 0 and 1 give the same lists, scores and counters (and the oracle's)."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(n_customers=130, n_vehicles=9, capacity=90, seed=21, slack=300, tw_seed=2)
    d_tw = sfa.build_cvrp(p, n_replicas=2)
    d_no = sfa.build_cvrp(_without_windows(p), n_replicas=2)
    d_tw.calculate_score(), d_no.calculate_score()
    assert d_tw.time_window_path(0) == "composed" and d_no.time_window_path(0) == "none"
    _run_and_compare(d_tw, [_oracle_model(oracle, p)], mode, 1000)
    _run_and_compare(d_no, [_oracle_model(oracle, p, windows=False)], mode, 1000)
    for r in range(2):
        assert d_tw.working_lists(0, r) == d_no.working_lists(0, r)
        a, b = d_tw.stats(r), d_no.stats(r)
        assert all(a[k] == b[k] for k in COUNTERS)
    assert (d_tw.calculate_score() == d_no.calculate_score()).all()
