"""GPU: LimitedNeighborhood around a leaf and around the root union, and Variable Neighborhood Descent over neighbourhoods that are
compositions, in the generic engine.  The oracle's union scheduler has no per-child budget, so the tests stand on tests/limited_mirror.py
(pinned on the oracle by tests/test_limited_mirror.py, which also asserts that the scripts of tests/limited_cases.py reach every edge):

1. sf_step_generate under every script's limits is the mirror's stream; every traced step of every script under HillClimbing /
   LateAcceptance x BestScore / AcceptedCount is the step mirror's: records, scores, doable and accepted flags, the leaf, the pick, the
   seven counters, committed score == full recalculation; fused launches end where the traced steps did;
2. limits that never bind leave a fused run under every acceptor of the generic engine bit for bit the unlimited run (and the oracle's);
3. VND: every step against the VND mirror, fused runs, solve_vnd, vnd_done_count, n_hoods = 0;
4. three replicas on their own seeds; one launch of more than one residency;
5. every refusal with its code, and the way back to the usual engine."""
import numpy as np
import pytest

import limited_cases as lc
import limited_mirror as lm

pytestmark = pytest.mark.gpu

R = 3
NEVER = 10 ** 6  # a limit no cursor of these models reaches
_memo = {}


def _t(moves):
    return np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1).tolist()


def _config(acceptor, forager, seed):
    import solverforge_amd as sfa

    return sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=lc.LA_SIZE, forager=forager, accepted_count_limit=lc.ACCEPTED_LIMIT, random_ties=False,
                            selection_order=lc.ORDER_RANDOM, random_seed=seed)


def _search_director(script, cfg, n_replicas=R, seed=lc.SEED, limits=True):
    d = lc.device_model(script, n_replicas)
    if limits:
        lc.apply_limits(d, script)
    d.configure(_config(cfg[0], cfg[1], seed))
    d.calculate_score()
    d.phase_start()
    return d


def _snapshot(d, script, r):
    st = d.stats(r)
    return (d.calculate_score()[r].tolist(), d.best_scores()[r].tolist(), lc.device_state(d, script, r), [st[k] for k in lm.COUNTERS])


def _check_step(d, script, r, rec, got, where):
    gm, gs, gf, gap, gmv = got
    cands = rec["candidates"][:rec["consumed"]]
    assert _t(gm) == [list(c["record"]) for c in cands], where
    assert ((gf & 1) != 0).tolist() == [c["doable"] for c in cands], where
    assert [tuple(row) for row, c in zip(gs.tolist(), cands) if c["doable"]] == [c["score"] for c in cands if c["doable"]], where
    assert ((gf & 2) != 0).tolist() == rec["accepted"], where
    assert (gf >> 8).tolist() == [c["child"] for c in cands], where  # the flags carry the global leaf index
    assert np.flatnonzero(gf & 4).tolist() == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), where
    if gap:
        assert list(int(x) for x in gmv.tolist()) == list(cands[rec["pick"]]["record"]), where
    assert tuple(d.calculate_score()[r].tolist()) == rec["score"], where


def _traced(oracle, name, cfg):
    """The script's first STEPS steps traced on replica 0 against the mirror; returns the snapshots of all replicas afterwards."""
    key = (name, cfg)
    if key in _memo:
        return _memo[key]
    script = lc.SEARCH[name]
    d = _search_director(script, cfg)
    o, mirror = lc.search_mirror(oracle, script, lc.SEED, *cfg)
    for step in range(lc.STEPS):
        got = d.solve_step_traced(replica=0, cap=1 << 13)
        rec = mirror.step()
        _check_step(d, script, 0, rec, got, (name, cfg, step))
        assert [d.stats(0)[k] for k in lm.COUNTERS] == [mirror.stats[k] for k in lm.COUNTERS], (name, cfg, step)
    assert (d.fresh_score() == d.calculate_score()).all()
    snap = _snapshot(d, script, 0)
    assert snap[1] == list(mirror.best_score) and snap[2] == lc.state_of(o, script)
    _memo[key] = [_snapshot(d, script, r) for r in range(R)]
    return _memo[key]


@pytest.mark.parametrize("name", list(lc.SEARCH))
def test_step_generate_is_the_mirrors_stream(oracle, name):
    script = lc.SEARCH[name]
    d = _search_director(script, lc.CONFIGS[0])
    o, mirror = lc.search_mirror(oracle, script, lc.SEED, *lc.CONFIGS[0])
    for step_index, seed, order in ((0, 1, 0), (5, 0x9E3779B97F4A7C15, 3), (17, 12345, 3)):
        gm, gs, gd = d.open_cursor(step_index, seed, order, replica=0, cap=1 << 13)
        pulls, children = mirror.stream(step_index, seed, order)
        want = [children[c][i] for c, i in pulls]
        assert _t(gm) == [[int(x) for x in m.tolist()] for m in want], (name, step_index)
        if want:
            sc, dv = o.evaluate_moves(np.array(want, dtype=children[0].dtype))
            assert gd.astype(bool).tolist() == dv.astype(bool).tolist()
            assert [row for row, ok in zip(gs.tolist(), dv) if ok] == [row[:2] for row, ok in zip(sc.tolist(), dv) if ok]


@pytest.mark.parametrize("cfg", lc.CONFIGS)
@pytest.mark.parametrize("name", list(lc.SEARCH))
def test_traced_steps_are_the_step_mirrors(oracle, name, cfg):
    _traced(oracle, name, cfg)


@pytest.mark.parametrize("name", list(lc.SEARCH))
def test_fused_launches_end_where_the_traced_steps_did(oracle, name):
    script = lc.SEARCH[name]
    for cfg in lc.CONFIGS:
        want = _traced(oracle, name, cfg)
        one = _search_director(script, cfg)
        one.solve_steps(lc.STEPS)
        two = _search_director(script, cfg)
        two.solve_steps(1)
        two.solve_steps(lc.STEPS - 1)
        for d in (one, two):
            assert [_snapshot(d, script, r) for r in range(R)] == want, (name, cfg)
            assert (d.fresh_score() == d.calculate_score()).all()
        # the acceptor's state (the late-acceptance history) shows in what follows: three more steps, fused and traced, end alike again
        one.solve_steps(3)
        for _ in range(3):
            two.solve_step_traced(replica=1, cap=1 << 13)
        assert [_snapshot(one, script, r) for r in range(R)] == [_snapshot(two, script, r) for r in range(R)], (name, cfg)


def _other_acceptor(d, acceptor, seed):
    import solverforge_amd as sfa
    from solverforge_amd.director import Acceptor

    if acceptor == Acceptor.TABU_SEARCH:
        d.configure_tabu(entity_tabu_size=3, move_tabu_size=5)
    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=lc.LA_SIZE, forager=0, accepted_count_limit=4, random_ties=True,
                                 selection_order=lc.ORDER_RANDOM, random_seed=seed))
    if acceptor == 3:
        d.configure_annealing(seed=seed)
    if acceptor == 4:
        d.configure_diversified(0.05)
    if acceptor == Acceptor.GREAT_DELUGE:
        d.configure_great_deluge(0.01)
    if acceptor == Acceptor.STEP_COUNTING_HILL_CLIMBING:
        d.configure_step_counting(5)


@pytest.mark.parametrize("acceptor", [0, 1, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("model", ["colouring", "jobshop", "cvrp"])
def test_limits_that_never_bind_are_the_identity(oracle, model, acceptor):
    if acceptor == 7 and model == "cvrp":
        model_leaves = ("list_change", "list_swap")  # TabuSearch covers the change and swap leaves
    else:
        model_leaves = lc.MODEL_LEAVES[model]
    script = {"model": model, "leaves": model_leaves, "order": lm.STRATIFIED_RANDOM, "child": {l: NEVER + l for l in range(len(model_leaves))},
              "root": 10 * NEVER, "weights": None}
    runs = []
    for limits in (False, True):
        d = lc.device_model(script, R)
        if limits:
            for l, lim in script["child"].items():
                d.limit_selector(l, lim)
            d.limit_union(script["root"])
        _other_acceptor(d, acceptor, 11)
        d.calculate_score()
        d.phase_start()
        d.solve_steps(12)
        d.solve_steps(13)
        runs.append([_snapshot(d, script, r) for r in range(R)])
        assert (d.fresh_score() == d.calculate_score()).all()
    assert runs[0] == runs[1]
    assert len({str(s[2]) for s in runs[0]}) > 1  # the replicas went apart: the comparison is not one run three times
    if acceptor == 1:  # the oracle itself on replica 0
        o = lc.oracle_model(oracle, script)
        o.configure(acceptor=1, la_size=lc.LA_SIZE, forager=0, limit=4, random_ties=True, selection_order=lc.ORDER_RANDOM, leaves=sum(lc.leaf_bits(script)), random_seed=11)
        o.set_sublist_sizes(*lc.SUBLIST_SIZES)
        o.phase_start()
        o.steps(25)
        assert runs[1][0][2] == lc.state_of(o, script) and runs[1][0][0] == [int(x) for x in o.score()[:2]]
        assert runs[1][0][3] == [o.stats()[k] for k in lm.COUNTERS]


# ---- Variable Neighborhood Descent -------------------------------------------------------------------------------------------------
def _vnd_director(script, n_replicas=R, seed=lc.SEED, grouped=True):
    d = lc.device_model(script, n_replicas)
    if grouped:
        lc.apply_limits(d, script)
    d.configure(_config(1, 0, seed))  # (the seed of the phase: the step seeds are drawn from random_seed + r)
    d.configure_vnd()
    d.calculate_score()
    d.phase_start()
    return d


def _vnd_snapshot(d, script, r):
    return _snapshot(d, script, r) + (d.vnd_state(r),)


def _vnd_traced(oracle, name, r=0):
    key = ("vnd", name, r)
    if key in _memo:
        return _memo[key]
    script = lc.VND[name]
    d = _vnd_director(script)
    o, mirror = lc.vnd_mirror(oracle, script, lc.SEED + r, *lc.device_state(d, script, r))
    steps = 0
    while not mirror.done and steps < script["steps"]:
        assert d.vnd_state(r) == mirror.state(), (name, steps)
        cur = mirror.current
        gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 13)
        rec = mirror.step()
        where = (name, r, steps)
        assert len(gm) == rec["cursor"] and _t(gm) == [[int(x) for x in m.tolist()] for m in rec["moves"]], where
        assert ((gf & 1) != 0).tolist() == rec["doable"] and (gf >> 8).tolist() == rec["children"], where
        assert [tuple(row) for row, ok in zip(gs.tolist(), rec["doable"]) if ok] == [sc for sc, ok in zip(rec["scores"], rec["doable"]) if ok], where
        accepted = [ok and sc > cur for sc, ok in zip(rec["scores"], rec["doable"])]
        assert ((gf & 2) != 0).tolist() == accepted, where
        assert np.flatnonzero(gf & 4).tolist() == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), where
        best = [sc for sc, ok in zip(rec["scores"], accepted) if ok]
        assert rec["ties"] == (best.count(max(best)) if best else 0), where
        assert tuple(d.calculate_score()[r].tolist()) == rec["score"], where
        assert [d.stats(r)[k] for k in lm.COUNTERS] == [mirror.stats[k] for k in lm.COUNTERS], where
        steps += 1
    assert d.vnd_state(r) == mirror.state() and d.vnd_state(r)["n"] == len(script["groups"])
    assert lc.device_state(d, script, r) == lc.state_of(o, script) and (d.fresh_score() == d.calculate_score()).all()
    _memo[key] = (steps, mirror.done, [_vnd_snapshot(d, script, q) for q in range(R)])
    return _memo[key]


@pytest.mark.parametrize("name", list(lc.VND))
def test_vnd_steps_are_the_vnd_mirrors(oracle, name):
    steps, done, _ = _vnd_traced(oracle, name)
    assert steps > 0 and (done or steps == lc.VND[name]["steps"])


@pytest.mark.parametrize("name", list(lc.VND))
def test_vnd_fused_ends_where_the_traced_run_did(oracle, name):
    script = lc.VND[name]
    steps, done, want = _vnd_traced(oracle, name)
    d = _vnd_director(script)
    d.solve_steps(steps)
    assert [_vnd_snapshot(d, script, r) for r in range(R)] == want
    two = _vnd_director(script)
    two.solve_steps(2)
    two.solve_steps(steps - 2)
    assert [_vnd_snapshot(two, script, r) for r in range(R)] == want
    assert d.vnd_done_count() == sum(1 for s in want if s[4]["done"])
    if done:
        sv = _vnd_director(script)
        assert sv.vnd_done_count() == 0
        assert sv.solve_vnd(500, steps_per_launch=5) == R == sv.vnd_done_count()
        assert all(sv.vnd_state(r)["done"] and sv.vnd_state(r)["k"] == sv.vnd_state(r)["n"] == len(script["groups"]) for r in range(R))
        assert _vnd_snapshot(sv, script, 0) == want[0]


@pytest.mark.parametrize("name", ["jobshop_three", "colouring_random"])
def test_vnd_without_groups_is_one_leaf_each(oracle, name):
    script = lc.VND[name]
    runs = []
    for mode in ("never_set", "cleared", "singletons"):
        d = lc.device_model(script, R)
        if mode == "cleared":
            d.set_vnd_neighborhoods(list(script["groups"]), script["orders"], script["limits"])
            d.set_vnd_neighborhoods([])
        if mode == "singletons":
            d.set_vnd_neighborhoods([1] * len(script["leaves"]))
        d.configure(_config(1, 0, lc.SEED))
        d.configure_vnd()
        d.calculate_score()
        d.phase_start()
        assert d.vnd_state(0)["n"] == len(script["leaves"])
        assert d.solve_vnd(500, steps_per_launch=7) == R
        runs.append([_vnd_snapshot(d, script, r) for r in range(R)])
    assert runs[0] == runs[1] == runs[2]
    import vnd_mirror as vm

    o = lc.oracle_model(oracle, script)
    ph = vm.VndPhase(o, lc.leaf_bits(script), lambda s: oracle.lib().sfo_step_seed(lc.SEED, s))
    ph.run()
    assert runs[0][0][2] == lc.state_of(o, script) and runs[0][0][3] == [ph.stats[k] for k in lm.COUNTERS]


# ---- replicas -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jobshop_cut_and_dry", "colouring_root_129", "cvrp_child_128"])
def test_three_replicas_against_their_own_mirrors(oracle, name):
    script, cfg = lc.SEARCH[name], lc.CONFIGS[3]
    ends = []
    for r in range(R):
        d = _search_director(script, cfg)
        o, mirror = lc.search_mirror(oracle, script, lc.SEED + r, *cfg)
        for step in range(lc.STEPS):
            got = d.solve_step_traced(replica=r, cap=1 << 13)
            _check_step(d, script, r, mirror.step(), got, (name, r, step))
        assert [d.stats(r)[k] for k in lm.COUNTERS] == [mirror.stats[k] for k in lm.COUNTERS]
        ends.append(str(lc.device_state(d, script, r)))
    assert len(set(ends)) == R
    for name_v in ("jobshop_three",):  # and under VND: replica 1 and 2 draw other offsets for the group
        for r in (1, 2):
            _vnd_traced(oracle, name_v, r)


def test_a_launch_of_more_than_one_residency(oracle):
    from test_gpu_large_launch import _cus

    script, cfg = lc.SEARCH["jobshop_cut_and_dry"], lc.CONFIGS[3]
    n = 32 * _cus() + 37
    d = _search_director(script, cfg, n_replicas=n)
    d.solve_steps(2)
    d.solve_steps(lc.STEPS - 2)
    assert (d.fresh_score() == d.calculate_score()).all()
    assert sum(d.stats(r)["step_count"] for r in (0, n // 2, n - 1)) == 3 * lc.STEPS
    for r in (0, 1, 63, 64, 32 * _cus() - 1, 32 * _cus(), n - 2, n - 1):
        o, mirror = lc.search_mirror(oracle, script, lc.SEED + r, *cfg)
        for _ in range(lc.STEPS):
            mirror.step()
        snap = _snapshot(d, script, r)
        assert snap[0] == list(mirror.current) and snap[1] == list(mirror.best_score) and snap[2] == lc.state_of(o, script), r
        assert snap[3] == [mirror.stats[k] for k in lm.COUNTERS], r


# ---- refusals and the way back ---------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back(oracle):
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    p = lc.problem("cvrp")
    # at the call: SF_ERR_INVALID
    d = sfa.build_cvrp(p, n_replicas=2, leaves=("list_change", "list_swap"))
    for bad in (lambda: d.limit_selector(2, 5), lambda: d.limit_selector(-1, 5), lambda: d.limit_selector(0, -2), lambda: d.limit_union(-2),
                lambda: d.set_vnd_neighborhoods([1]), lambda: d.set_vnd_neighborhoods([1, 2]), lambda: d.set_vnd_neighborhoods([2], [5]),
                lambda: d.set_vnd_neighborhoods([2], [0], [-2]), lambda: d.set_vnd_neighborhoods([0, 2])):
        with pytest.raises(sfa.SolverForgeError, match="INVALID"):
            bad()
    d.limit_selector(0, 1 << 40)  # a limit no 32-bit pull count reaches is none: the context stays on its usual engine
    d.limit_selector(0, None)
    # a forced engine under a limit, and under a grouping
    for engine in (1, 2):
        for how in ("leaf", "root", "groups"):
            dl = sfa.build_cvrp(p, n_replicas=2, leaves=("nearby_change", "nearby_swap"))
            dl.set_engine(engine)
            if how == "leaf":
                dl.limit_selector(1, 10)
            elif how == "root":
                dl.limit_union(10)
            else:
                dl.set_vnd_neighborhoods([2])
            dl.configure(_config(1, 0, 3))
            dl.calculate_score()
            dl.phase_start()
            with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*generic engine only"):
                dl.solve_steps(2)
    # a limit around a union that holds a ruin leaf, a scalar ruin leaf or the critical-path leaf
    q = datasets.make_precedence_shop(4, 3, seed=2)
    g = lc.problem("colouring")

    def with_scalar_ruin():
        ds = sfa.build_graph_coloring(g, n_replicas=2, leaves=("change",))
        ds.add_scalar_ruin_selector(0)
        return ds

    for build, reason in ((lambda: sfa.build_cvrp(p, n_replicas=2, leaves=("list_change", "ruin")), "list ruin leaf"), (with_scalar_ruin, "scalar ruin leaf"),
                          (lambda: sfa.build_precedence_shop(q, n_replicas=2, leaves=("precedence", "list_change")), "critical-path leaf")):
        for how in ("leaf", "root"):
            dr = build()
            if how == "leaf":
                dr.limit_selector(0, 10)
            else:
                dr.limit_union(10)
            dr.configure(_config(1, 0, 3))
            dr.calculate_score()
            dr.phase_start()
            with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*limited neighbourhood.*" + reason):
                dr.solve_steps(2)
            with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*limited neighbourhood.*" + reason):
                dr.open_cursor(0, 1, 3)
    # more leaves than a union holds
    dm = sfa.build_cvrp(p, n_replicas=2, leaves=("list_change",) * 13)
    dm.limit_selector(12, 5)
    dm.configure(_config(1, 0, 3))
    dm.calculate_score()
    dm.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*too many leaves"):
        dm.solve_steps(2)
    # the way back: limits removed, grouping cleared -> the usual engine (the nearby pair's wave engine, the scalar engine), and the oracle again
    for model in ("cvrp", "colouring"):
        script = {"model": model, "leaves": ("nearby_change", "nearby_swap") if model == "cvrp" else ("change", "swap"), "child": {}}
        if model == "cvrp":
            db = sfa.build_cvrp(p, n_replicas=2, leaves=script["leaves"], max_nearby=6)
        else:
            db = lc.device_model(script, 2)
        db.limit_selector(0, 7)
        db.limit_union(9)
        db.set_vnd_neighborhoods([2])
        db.configure(_config(1, 0, 17))
        db.calculate_score()
        db.phase_start()
        gm, _, gf, _, _ = db.solve_step_traced(replica=0, cap=1 << 13)
        assert len(gm) <= 9 and (gf >> 8).tolist().count(0) <= 7
        db.limit_selector(0, None)
        db.limit_union(None)
        db.set_vnd_neighborhoods([])
        db.phase_start()
        values, lists = lc.device_state(db, script, 0)
        if model == "cvrp":
            o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], lists)
        else:
            o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], values)
        o.configure(acceptor=1, la_size=lc.LA_SIZE, forager=0, limit=lc.ACCEPTED_LIMIT, random_ties=False, selection_order=lc.ORDER_RANDOM,
                    leaves=sum(lc.LEAF_BITS[x] for x in script["leaves"]), max_nearby=6, random_seed=17)
        o.phase_start()
        gm, gs, gf, gap, gmv = db.solve_step_traced(replica=0, cap=1 << 13)
        om, os_, of, oap, omv = o.step_traced()
        assert len(gm) == len(om) > 0 and _t(gm) == _t(om) and (gf == of).all() and (gs == os_[:, :2]).all() and gap == oap
        db.solve_steps(5)
        o.steps(5)
        assert lc.device_state(db, script, 0) == lc.state_of(o, script)
