"""GPU parity tests (through the C ABI) at the edges of the host range checks that pick the narrow-arithmetic kernels: the u32 / u16
matrix copies, the 16-bit ruin leg tables, 32-bit trial deltas (`small32`: wave-engine MODE 2, the FAST generic kernels and their
32-bit pre-evaluated ring, the list-preserving ruin recreate), LateAcceptance as one 64-bit key with clamped thresholds, and one-byte
scalar values.  Every case sits on one side of one gate, asserts the side the library took (sf_list_arith_flags / sf_list_wave_layout),
then compares against the CPU oracle bit for bit: the trial scores of a whole cursor, traced steps, a fused window (lists, scores,
best score, counters) and fresh_score.

Edge values come from the host's own inequalities (csrc/sf_api.hip, build_list_model):
  mat32   max_finite < 0xFFFFFFFF                  -> last 0xFFFFFFFE, first out 0xFFFFFFFF
  mat16 / leg16   max_finite < 0xFFFF              -> last 0xFFFE, first out 0xFFFF
  small32  max_finite < 2^26 and |w_dist| * 8 * (max_leg + 1) < 2^29
           -> with w_dist = 1: last 2^26 - 2, first out 2^26 - 1; for a max leg the last w_dist is (2^29 - 1) // (8 (max_leg + 1))
           demand abs_sum, |capacity| < 2^28 and |w_cap| * 2 * (abs_sum + |capacity| + 1) < 2^29
  FAST + ruin   leg16 && V <= 128 && small32 && mat16 (+ n_cap, dim <= 32767)
  int8 values   n_values <= 127 (scalar engine); n_values <= 127 && n >= 1024 (generic engine); n_values > 32767 refused"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAF_BITS = {"nearby_change": 16, "nearby_swap": 32, "list_change": 4, "list_swap": 8, "list_reverse": 64,
             "sublist_change": 128, "sublist_swap": 256, "kopt": 512, "ruin": 1024}
DEFAULT_POLICY = ("nearby_change", "nearby_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt", "ruin")
SIX_LEAVES = DEFAULT_POLICY[:-1]
NEARBY = ("nearby_change", "nearby_swap")
COUNTERS = ["step_count", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations"]
UNREACHABLE = np.iinfo(np.int64).max
MAXN = 10

U16_LAST, U16_OUT = 0xFFFE, 0xFFFF
S32_LAST, S32_OUT = (1 << 26) - 2, (1 << 26) - 1
U32_LAST, U32_OUT = 0xFFFFFFFE, 0xFFFFFFFF


def _t(moves):
    return np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1)


def _w_dist_last(max_leg):
    """The largest distance weight the small32 check admits for a matrix whose largest leg is max_leg."""
    return ((1 << 29) - 1) // (8 * (max_leg + 1))


def _w_cap_last(dem, cap):
    return ((1 << 29) - 1) // (2 * (dem + abs(cap) + 1))


def _top_problem(top, n=60, v=6, cap=40, seed=5, affine=True):
    """make_cvrp's instance with every off-diagonal leg moved to the top of [0, top - 1] by an increasing affine map (nearby
    lists and ties keep their meaning; most trial deltas are sums of near-maximal legs), then `top` itself placed on two legs
    that the starting routes use: depot -> first customer of route 0, and the first leg inside route 1."""
    from solverforge_amd import datasets

    p = datasets.make_cvrp(n, v, cap, seed=seed)
    m = p["matrix"]
    mx = int(m.max())
    lo = top - 1
    s = max(1, (lo // 4) // mx) if affine else lo // mx
    base = lo - s * mx if affine else 0
    q = (base + m * s).astype(np.int64)
    np.fill_diagonal(q, 0)
    r0, r1 = p["routes"][0], p["routes"][1]
    for a, b in ((p["depot"], r0[0]), (r1[0], r1[1])):
        q[a, b] = q[b, a] = top
    assert int(q.max()) == top and (q == q.T).all()
    p["matrix"] = q
    return p


def _mk(oracle, p, leaves, engine=None, weights=(1, 1, 1), n_replicas=1, seed=3, la=400, limit=256, ruin=(2, 5, 10)):
    import solverforge_amd as sfa

    d = sfa.build_cvrp(p, n_replicas=n_replicas, leaves=leaves, ruin=ruin, max_nearby=MAXN, weights=weights)
    if engine is not None:
        d.set_engine(engine)
    o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=weights)
    o.configure(leaves=sum(LEAF_BITS[x] for x in leaves), random_seed=seed, max_nearby=MAXN, la_size=la, limit=limit)
    if "ruin" in leaves:
        o.set_ruin(ruin[0], ruin[1], ruin[2], variable_name="visits")
    d.configure(sfa.SolverConfig(random_seed=seed, late_acceptance_size=la, accepted_count_limit=limit))
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    return d, o


def _model_flags(d, **want):
    model, _ = d.arith_flags()
    for k, v in want.items():
        assert model[k] == v, (k, model)


def _cursor(oracle, d, p, leaves, weights, seed, ruin=(2, 5, 10)):
    """Every candidate of step 0's cursor and its trial score (after phase start: the ruin leaf's stream is seeded there).  The
    oracle enumerates on a twin model, so that the run it is compared with afterwards has consumed nothing."""
    ot = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=weights)
    ot.configure(leaves=sum(LEAF_BITS[x] for x in leaves), random_seed=seed, max_nearby=MAXN)
    if "ruin" in leaves:
        ot.set_ruin(ruin[0], ruin[1], ruin[2], variable_name="visits")
    ot.phase_start()
    step_seed = int(oracle.lib().sfo_step_seed(seed, 0))
    gm, gs, gd = d.open_cursor(0, step_seed, selection_order=3, cap=1 << 18)
    om = ot.enumerate(0, 0, step_seed, 3)
    # ruin candidates are priced by the traced steps (their draws come from the per-solve stream, not the step's context)
    kg, ko = gm["kind"] != 8, om["kind"] != 8
    gm, gs, gd, om = gm[kg], gs[kg], gd[kg], om[ko]
    assert len(gm) == len(om) > 0
    assert (_t(gm) == _t(om)).all()
    os_, od = ot.evaluate_moves(om)
    assert (gd == od).all()
    assert (gs == os_[:, :2]).all()


def _traced(d, o, n):
    for step in range(n):
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 18)
        om, os_, of, oap, omv = o.step_traced()
        assert len(gm) == len(om), step
        assert (_t(gm) == _t(om)).all(), step
        assert (gs == os_[:, :2]).all(), step
        assert (gf == of).all(), step
        assert gap == oap, step
        if gap:
            assert tuple(gmv) == tuple(omv), step
        assert d.working_lists(0, 0) == o.get_lists(0), step


def _fused(d, o, chunks):
    for n in chunks:
        d.solve_steps(n)
    o.steps(sum(chunks))
    assert d.working_lists(0, 0) == o.get_lists(0)
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    assert (d.best_scores()[0] == o.best_score()[:2]).all()
    gst, ost = d.stats(0), o.stats()
    for k in COUNTERS:
        assert gst[k] == ost[k], k
    assert (d.fresh_score()[0] == o.score()[:2]).all()
    assert (d.fresh_score()[0] == d.calculate_score()[0]).all()


def _flags_by_top(top):
    return dict(mat32=top < 0xFFFFFFFF, mat16=top < 0xFFFF, leg16=top < 0xFFFF, small32=top <= S32_LAST)


TOPS = [U16_LAST, U16_OUT, S32_LAST, S32_OUT, U32_LAST, U32_OUT]


# ---- leg magnitudes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", TOPS)
def test_leg_edges_wave_engine(oracle, top):
    """The two-leaf nearby union on the wave engine: COMPACT (u16 matrix) -> MODE 2 (32-bit deltas) -> MODE 1 (64-bit) -> general."""
    p = _top_problem(top)
    d, o = _mk(oracle, p, NEARBY, engine=2, seed=3)
    want = _flags_by_top(top)
    _model_flags(d, **want)
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, NEARBY, (1, 1, 1), 3)
    _traced(d, o, 20)
    _fused(d, o, (15, 15))
    mode, _ = d.wave_layout()
    if not want["mat32"]:
        assert mode == 0, mode
    elif not want["small32"]:
        assert mode == 1, mode
    elif not want["mat16"]:
        assert mode == 2, mode
    else:
        assert mode >= 3, mode


@pytest.mark.parametrize("top", [U16_LAST, U16_OUT])
def test_leg_edges_block_engine(oracle, top):
    p = _top_problem(top, seed=7)
    d, o = _mk(oracle, p, NEARBY, engine=1, seed=4)
    _model_flags(d, **_flags_by_top(top))
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, NEARBY, (1, 1, 1), 4)
    _traced(d, o, 20)
    _fused(d, o, (20,))


@pytest.mark.parametrize("top", TOPS)
def test_leg_edges_generic_engine_seven_leaves(oracle, top):
    """The seven-leaf default list policy: FAST + list-preserving ruin (0xFFFE) -> general kernel with the matrix-gather recreate."""
    p = _top_problem(top, seed=11)
    d, o = _mk(oracle, p, DEFAULT_POLICY, seed=2)
    want = _flags_by_top(top)
    _model_flags(d, **want)
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, DEFAULT_POLICY, (1, 1, 1), 2)
    _traced(d, o, 20)
    _fused(d, o, (15, 15))
    _, gen = d.arith_flags()
    fast = want["leg16"] and want["small32"] and want["mat16"]
    assert gen["fast"] == fast and gen["node_global"] == fast and gen["ring32"] == fast, gen
    assert gen["ruin"] == (3 if fast else (2 if want["leg16"] else 1)), gen
    assert gen["value_bytes"] == 2


@pytest.mark.parametrize("top", [S32_LAST, S32_OUT])
def test_small32_edge_fast_ring(oracle, top):
    """The six leaves without ruin keep the FAST generic kernel on both sides; its 32-bit pre-evaluated ring only below the edge."""
    p = _top_problem(top, seed=12)
    d, o = _mk(oracle, p, SIX_LEAVES, seed=6)
    _model_flags(d, **_flags_by_top(top))
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, SIX_LEAVES, (1, 1, 1), 6)
    _traced(d, o, 20)
    _fused(d, o, (15, 15))
    _, gen = d.arith_flags()
    assert gen["fast"] and gen["ruin"] == 0, gen
    assert gen["ring32"] == (top == S32_LAST), gen


@pytest.mark.parametrize("top", [U32_LAST, U32_OUT])
def test_mat32_edge_constructions(oracle, top):
    """Cheapest insertion, Clarke-Wright savings and route-local k-opt read the u32 copy when it exists."""
    p = _top_problem(top, seed=14)
    p["routes"] = [[] for _ in p["routes"]]
    import solverforge_amd as sfa

    for phase in ("cheapest", "savings"):
        d = sfa.build_cvrp(p, n_replicas=1)
        o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
        d.calculate_score()
        _model_flags(d, mat32=top < 0xFFFFFFFF, mat16=False)
        if phase == "cheapest":
            d.construct_list_cheapest(0, p["customers"])
            o.construct_list_cheapest(p["customers"])
        else:
            d.construct_list_clarke_wright(0, p["customers"], 1)
            o.construct_list_clarke_wright(p["customers"], 1)
        assert d.working_lists(0, 0) == o.get_lists(0), phase
        assert (d.calculate_score()[0] == o.score()[:2]).all(), phase
        cs = d.construct_list_k_opt(0, 2, 1)
        o.construct_list_k_opt(2, 1)
        assert d.working_lists(0, 0) == o.get_lists(0), phase
        assert (cs[0] == o.score()[:2]).all(), phase
        assert (d.fresh_score()[0] == o.score()[:2]).all(), phase
        d.close()


def test_real_0xfffe_leg_meets_the_sentinel(oracle):
    """A genuine 0xFFFE leg next to UNREACHABLE and negative legs in the same routes: the 16-bit leg tables hold 0xFFFE as a value and
    0xFFFF as the sentinel (-> MAX_SAFE_LEG_COST) in one ruin trial.  Not every leg is finite, so no 32-bit deltas."""
    p = _top_problem(U16_LAST, n=40, v=4, seed=3)
    m, r0, r1 = p["matrix"], p["routes"][0], p["routes"][1]
    for a, b, val in [(r0[0], r0[1], UNREACHABLE), (r0[1], r0[2], -3), (r1[1], r1[2], UNREACHABLE), (r1[2], r1[3], U16_LAST),
                      (r0[2], r1[0], UNREACHABLE)]:
        m[a, b] = m[b, a] = val
    d, o = _mk(oracle, p, DEFAULT_POLICY, seed=5, ruin=(1, 6, 16))
    _model_flags(d, mat32=True, mat16=True, leg16=True, small32=False)
    d.phase_start()
    o.phase_start()
    _traced(d, o, 30)
    _fused(d, o, (20, 20))
    _, gen = d.arith_flags()
    assert not gen["fast"] and gen["ruin"] == 2, gen


# ---- weights and loads at the small32 check --------------------------------------------------------------------------------------
def _load_problem(dem_total, cap, n=48, v=3, seed=8):
    """Long routes (16 customers each) whose demands sum to dem_total (None: make_cvrp's own); capacity `cap`."""
    p = _top_problem(U16_LAST, n=n, v=v, cap=cap, seed=seed)
    if dem_total is None:
        return p
    dem = p["demands"].astype(np.int64)
    scaled = dem * (dem_total // int(dem.sum()))
    scaled[1] += dem_total - int(scaled.sum())
    assert int(scaled.sum()) == dem_total and scaled.max() < (1 << 31)
    p["demands"] = scaled.astype(np.int32)
    return p


def _weight_cases():
    wd = _w_dist_last(U16_LAST)
    # (name, dem_total, capacity, weights, small32)
    dem = 5_000_000
    cap = 1_600_000
    wc = _w_cap_last(dem, cap)
    near = (1 << 28) - 2 - 40_000_000  # abs_sum + capacity + 1 == 2^28 - 1: the last admitted with w_cap = 1
    return [
        ("w_dist_last", None, 90, (1, 1, wd), True),
        ("w_dist_out", None, 90, (1, 1, wd + 1), False),
        ("w_cap_last", dem, cap, (1, wc, 1), True),
        ("w_cap_out", dem, cap, (1, wc + 1, 1), False),
        ("load_2^28_last", near, 40_000_000, (1, 1, 1), True),
        ("load_2^28_out", near, 40_000_001, (1, 1, 1), False),
    ]


@pytest.mark.parametrize("case", _weight_cases(), ids=lambda c: c[0])
def test_small32_weight_and_load_edges(oracle, case):
    """Distance / capacity weight at the last admitted value and one more; demand abs_sum + capacity one below and at 2^28.  Six-element
    ruins on 16-customer routes: the largest int32 sum of ruin_trial_v2 (12 legs x w_dist + the capacity term)."""
    name, dem_total, cap, weights, small = case
    p = _load_problem(dem_total, cap)
    assert sum(len(r) for r in p["routes"]) == 48
    d, o = _mk(oracle, p, DEFAULT_POLICY, weights=weights, seed=7, ruin=(6, 6, 10))
    _model_flags(d, mat16=True, leg16=True, small32=small)
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, DEFAULT_POLICY, weights, 7, ruin=(6, 6, 10))
    _traced(d, o, 20)
    _fused(d, o, (15, 15))
    _, gen = d.arith_flags()
    assert gen["fast"] == small and gen["ruin"] == (3 if small else 2), gen


@pytest.mark.parametrize("case", _weight_cases()[:2], ids=lambda c: c[0])
def test_small32_weight_edges_wave_engine(oracle, case):
    name, dem_total, cap, weights, small = case
    p = _load_problem(dem_total, cap)
    d, o = _mk(oracle, p, NEARBY, engine=2, weights=weights, seed=9)
    _model_flags(d, small32=small)
    d.phase_start()
    o.phase_start()
    _cursor(oracle, d, p, NEARBY, weights, 9)
    _traced(d, o, 15)
    _fused(d, o, (20,))
    mode, _ = d.wave_layout()
    assert (mode >= 2) == small and mode >= 1, mode


# ---- LateAcceptance as one 64-bit key ----------------------------------------------------------------------------------------------
def test_late_acceptance_threshold_clamp(oracle):
    """Legs up to 2^26 - 2 (MODE 2 of the wave engine: level deltas in int32, the LA threshold late - current clamped to int32 and
    the two levels packed into one 64-bit key).  The oracle's per-step scores show that |late - current| on the soft level passed
    2^31 (the clamp was live); the fused run in three launches equals the oracle step for step.  The hard gap of this model is
    bounded by w_cap * abs_sum < 2^28 whenever small32 holds, so the -2^30 hard clamp cannot be reached by a CVRP; the run takes the
    largest capacity weight the check admits and asserts the hard gap it did reach."""
    from solverforge_amd import datasets

    p = datasets.make_cvrp(200, 10, 90, seed=13)
    m = p["matrix"]
    q = (m * (S32_LAST // int(m.max()))).astype(np.int64)
    r0 = p["routes"][0]
    q[p["depot"], r0[0]] = q[r0[0], p["depot"]] = S32_LAST
    p["matrix"] = q
    dem = int(np.abs(p["demands"]).sum())
    wc = _w_cap_last(dem, p["capacity"])
    weights = (1, wc, 1)
    steps = 480
    ot = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], q, p["customers"], p["routes"], weights=weights)
    ot.configure(leaves=16 | 32, random_seed=2, max_nearby=MAXN, la_size=400, limit=256)
    ot.phase_start()
    sc = [ot.score()[:2].copy()]
    for _ in range(steps):
        ot.steps(1)
        sc.append(ot.score()[:2].copy())
    sc = np.array(sc)
    # step t (1-based) compares against late = the score after step t - 400 (the phase's start score while t <= 400) and current
    late = sc[np.maximum(np.arange(1, steps + 1) - 400, 0)]
    gap = late - sc[:-1]
    assert np.abs(gap[:, 1]).max() > (1 << 31), np.abs(gap[:, 1]).max()
    assert gap[:, 0].min() < -(1 << 20), gap[:, 0].min()

    d, o = _mk(oracle, p, NEARBY, engine=2, weights=weights, seed=2)
    _model_flags(d, mat32=True, mat16=False, small32=True)
    d.phase_start()
    o.phase_start()
    _fused(d, o, (100, 200, 180))
    assert (d.calculate_score()[0] == sc[-1]).all()
    mode, _ = d.wave_layout()
    assert mode == 2, mode


# ---- FAST + ruin ---------------------------------------------------------------------------------------------------------------------
def test_fast_ruin_at_size(oracle):
    """CVRP-1000 / 100 routes, the seven default leaves, LA(400) + AcceptedCount(256), 4 replicas, 40 fused steps in two launches:
    the FAST + ruin instantiation with the node -> slot table in HBM; replica 0 against the oracle, every replica's incremental score
    against a full recalculation."""
    from solverforge_amd import datasets

    p = datasets.make_cvrp(1000, 100, 55, seed=0)
    d, o = _mk(oracle, p, DEFAULT_POLICY, n_replicas=4, seed=0)
    _model_flags(d, mat32=True, mat16=True, leg16=True, small32=True)
    d.phase_start()
    o.phase_start()
    _fused(d, o, (20, 20))
    _, gen = d.arith_flags()
    assert gen["fast"] and gen["node_global"] and gen["ring32"] and gen["ruin"] == 3, gen
    sc = d.calculate_score()
    assert (d.fresh_score() == sc).all()
    for r in range(4):
        assert sorted(c for rt in d.working_lists(0, r) for c in rt) == list(range(1, 1001)), r


@pytest.mark.parametrize("V", [64, 65, 128, 129])
def test_fast_ruin_route_count_edges(oracle, V):
    """V = 64 / 65: ruin_trial_v2 goes from one 64-lane pass over the lists to two; 128 is the last FAST + ruin route count, 129 takes the
    general instantiation (16-bit leg tables).  Empty and one-element routes included."""
    p = _top_problem(U16_LAST, n=3 * V, v=V, cap=25, seed=V)
    routes = p["routes"]
    moved = routes[1] + routes[3][1:]
    routes[1], routes[3] = [], routes[3][:1]
    routes[0] = routes[0] + moved
    d, o = _mk(oracle, p, DEFAULT_POLICY, seed=1)
    _model_flags(d, mat16=True, leg16=True, small32=True)
    d.phase_start()
    o.phase_start()
    _traced(d, o, 10)
    _fused(d, o, (15, 15))
    _, gen = d.arith_flags()
    assert gen["fast"] == (V <= 128), gen
    assert gen["ruin"] == (3 if V <= 128 else 2), gen


# ---- one-byte scalar values --------------------------------------------------------------------------------------------------------
def _st(moves):
    return np.stack([moves["kind"], moves["a"], moves["b"], moves["value"]], axis=1)


@pytest.mark.parametrize("k", [126, 127, 128])
def test_scalar_value_bytes_graph_coloring(oracle, k):
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    g = datasets.make_graph(300, 3000, k, seed=k)
    r = datasets.stream(k + 5, 300)
    g["colors"] = (r % np.uint64(k + 1)).astype(np.int64) - 1
    g["colors"][::7] = k - 1  # the top colour in use from the start
    d = sfa.build_graph_coloring(g)
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    bits = oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    o.configure(acceptor=1, la_size=5, forager=0, limit=64, leaves=bits, random_seed=9)
    d.configure(sfa.SolverConfig(acceptor=1, late_acceptance_size=5, forager=0, accepted_count_limit=64, random_seed=9))
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    d.phase_start()
    o.phase_start()
    gm, gs, gd = d.open_cursor(0, 17, selection_order=3, cap=1 << 17)
    om = o.enumerate(0, 0, 17, 3)
    assert len(gm) == len(om) > 0 and (_st(gm) == _st(om)).all()
    os_, od = o.evaluate_moves(om)
    assert (gd == od).all() and (gs == os_[:, :2]).all()
    assert (om["value"] >= k - 2).any()
    for step in range(20):
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 17)
        om, os_, of, oap, omv = o.step_traced()
        assert len(gm) == len(om) and (_st(gm) == _st(om)).all() and (gf == of).all() and (gs == os_[:, :2]).all(), step
        assert gap == oap, step
    d.solve_steps(40)
    o.steps(40)
    vals = d.working_values(0, 0)
    assert (vals == o.get_vars(0, 0)).all()
    assert vals.max() >= k - 3
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.best_scores()[0] == o.best_score()[:2]).all()
    assert (d.fresh_score()[0] == o.score()[:2]).all()
    for kk in COUNTERS:
        assert d.stats(0)[kk] == o.stats()[kk], kk
    model, _ = d.arith_flags()
    assert model["scalar_value_bytes"] == (1 if k <= 127 else 2), model


def _jobshop(n_jobs, n_machines, seed):
    from solverforge_amd import datasets

    p = datasets.make_jobshop(n_jobs, n_machines)
    n = p["n_ops"]
    r = datasets.stream(seed, 3 * n)
    p["machine_idx"] = (r[:n] % np.uint64(n_machines + 1)).astype(np.int64) - 1
    p["machine_idx"][::5] = n_machines - 1
    seqs = [[] for _ in range(n_machines)]
    for op in range(n):
        where = int(r[n + op] % np.uint64(n_machines + 2))
        if where < n_machines:
            seqs[where].append(op)
    p["sequences"] = seqs
    return p


@pytest.mark.parametrize("n_machines", [127, 128])
def test_scalar_value_bytes_generic_engine(oracle, n_machines):
    """A mixed model of >= 1024 scalar entities: one-byte values at 127 values, two bytes at 128 (the generic engine)."""
    import solverforge_amd as sfa

    p = _jobshop(9, n_machines, seed=4)
    assert p["n_ops"] >= 1024
    d = sfa.build_jobshop(p, n_replicas=1, bendable=False)
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=False)
    bits = oracle.LEAF_LIST_CHANGE | oracle.LEAF_LIST_SWAP | oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    o.configure(acceptor=1, la_size=5, forager=0, limit=12, leaves=bits, random_seed=6)
    d.configure(sfa.SolverConfig(acceptor=1, late_acceptance_size=5, forager=0, accepted_count_limit=12, random_seed=6))
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    d.phase_start()
    o.phase_start()
    for step in range(4):
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 18)
        om, os_, of, oap, omv = o.step_traced()
        assert len(gm) == len(om) and (_t(gm) == _t(om)).all() and (gf == of).all() and (gs == os_[:, :2]).all(), step
        assert gap == oap and (not gap or tuple(gmv) == tuple(omv)), step
    d.solve_steps(20)
    o.steps(20)
    assert (d.working_values(0, 0) == o.get_vars(0, 0)).all()
    assert d.working_lists(1, 0) == o.get_lists(1)
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()
    _, gen = d.arith_flags()
    assert gen["value_bytes"] == (1 if n_machines <= 127 else 2), gen


@pytest.mark.parametrize("k", [32767, 32768])
def test_scalar_value_range_limit(oracle, k):
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    g = datasets.make_graph(64, 200, k, seed=1)
    r = datasets.stream(3, 64)
    g["colors"] = (r % np.uint64(k)).astype(np.int64)
    g["colors"][0] = k - 1
    d = sfa.build_graph_coloring(g)
    if k > 32767:
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
            d.calculate_score()
        return
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    o.configure(acceptor=1, la_size=5, forager=0, limit=16, leaves=oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, random_seed=2)
    d.configure(sfa.SolverConfig(acceptor=1, late_acceptance_size=5, forager=0, accepted_count_limit=16, random_seed=2))
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    d.phase_start()
    o.phase_start()
    d.solve_steps(10)
    o.steps(10)
    assert (d.working_values(0, 0) == o.get_vars(0, 0)).all()
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()
    assert d.arith_flags()[0]["scalar_value_bytes"] == 2
