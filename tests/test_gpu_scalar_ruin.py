"""GPU: the scalar ruin-and-recreate leaf (sf_selector_add_scalar_ruin, csrc/sf_scalar_ruin.h) in the generic engine, bit-exact through
the C ABI against tests/scalar_ruin_mirror.py (pinned on the CPU by tests/test_scalar_ruin_mirror.py) over oracle models:

1. the leaf alone: the scripts of tests/scalar_ruin_cases.py step by step -- batch table, records, scores, flags, pick, counters, values;
2. the trial scores against sf_step_evaluate_compound over the table's edits;
3. unions with the change / swap leaves (Sequential, StratifiedRandom) and the mixed job shop beside a list change leaf;
4. fused launches, several replicas, a launch of many residencies;
5. sf_step_generate (a dry run that does not advance the stream), every refusal with its message, the way back."""
import numpy as np
import pytest

import scalar_ruin_cases as rc
import scalar_ruin_mirror as rm

pytestmark = pytest.mark.gpu

NAMES = list(rc.SCRIPTS)
_memo = {}


def _t(moves):
    return [tuple(int(x) for x in row) for row in np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1)]


def _start(name, n_replicas=1, **kw):
    d = rc.device_model(name, n_replicas, **{k: v for k, v in kw.items() if k in ("before", "after", "leaf")})
    rc.configure(d, name, **{k: v for k, v in kw.items() if k in ("search", "order", "union")})
    d.calculate_score()
    d.phase_start()
    return d


def _snapshot(d, r=0):
    st = d.stats(r)
    return (d.calculate_score()[r].tolist(), d.best_scores()[r].tolist(), d.working_values(0, 0, replica=r).tolist(), [st[k] for k in rm.COUNTERS])


def _mirror_snapshot(search):
    return (list(search.current), list(search.best_score), search.leaf.values(), [search.stats[k] for k in rm.COUNTERS])


def _check_step(d, search, r, where, cross_check=False):
    """One traced step of replica r against one mirror step."""
    before = d.working_values(0, 0, replica=r).tolist()
    gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 12)
    table = d.scalar_ruin_table(r)
    rec = search.step()
    assert table == rm.public_table(rec["table"]), where
    want = rec["candidates"][:rec["consumed"]]
    assert _t(gm) == [c["record"] for c in want], where
    assert ((gf & 1) != 0).tolist() == [c["doable"] for c in want], where
    assert [tuple(row) for row, c in zip(gs.tolist(), want) if c["doable"]] == [c["score"] for c in want if c["doable"]], where
    assert ((gf & 2) != 0).tolist() == rec["accepted"], where
    assert np.flatnonzero(gf & 4).tolist() == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), where
    if gap:
        assert tuple(int(x) for x in gmv) == want[rec["pick"]]["record"], where
    assert _snapshot(d, r) == _mirror_snapshot(search), where
    assert (d.fresh_score() == d.calculate_score()).all(), where
    return before, rec


def _traced(oracle, name):
    if name not in _memo:
        d = _start(name)
        o, search = rc.search_of(oracle, name)
        assert tuple(d.calculate_score()[0].tolist()) == search.current
        recs = []
        for step in range(rc.SCRIPTS[name]["steps"]):
            recs.append(_check_step(d, search, 0, (name, step)))
        _memo[name] = (recs, _snapshot(d), None)  # (results only: a device context kept to interpreter exit would be destroyed after the HIP runtime)
        d.close()
    return _memo[name]


@pytest.mark.parametrize("name", NAMES)
def test_leaf_alone_matches_the_mirror(oracle, name):
    recs, snap, _ = _traced(oracle, name)
    assert len(recs) == rc.SCRIPTS[name]["steps"] == snap[3][0]
    if name == "required_limit_zero":  # nothing emitted, nothing counted but the steps
        assert snap[3] == [3, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ["colouring_ci", "colouring_original", "assignment_range"])
def test_trial_scores_are_the_compound_evaluation(oracle, name):
    """Every emitted batch of three steps: its result as edits, scored by sf_step_evaluate_compound from the state before the step."""
    d = _start(name)
    o, search = rc.search_of(oracle, name)
    checked = 0
    for step in range(3):
        before = d.working_values(0, 0, replica=0).tolist()
        d.open_cursor(search.step_index, oracle.lib().sfo_step_seed(rc.SCRIPTS[name]["seed"], search.step_index), selection_order=rc.SCRIPTS[name]["order"])
        mrec = search.step(dry_run=True)
        rows = d.scalar_ruin_table(0)
        assert rows == rm.public_table(mrec["table"])
        for row, mrow in zip(rows, mrec["table"]):
            edits = [(e, v) for e, v in zip(row["entities"], row["values"] or []) if before[e] != v]
            if not row["emitted"] or not edits:
                continue
            sc, ok = d.evaluate_candidates([edits])
            assert ok[0] and tuple(sc[0].tolist()) == mrow["score"], (name, step, row)
            checked += 1
        _check_step(d, search, 0, (name, step))
    assert checked > 0


@pytest.mark.parametrize("before,after", [((), (1,)), ((1, 2), ())])
def test_sequential_union(oracle, before, after):
    name = "colouring_ff"
    d = _start(name, before=before, after=after, union=0, search=(rc.HC, rc.BEST))  # (BestScore: the whole union is pulled, every child to its end)
    o, search = rc.search_of(oracle, name, before=before, after=after, search=(rc.HC, rc.BEST))
    kinds = set()
    for step in range(4):
        _, rec = _check_step(d, search, 0, (before, after, step))
        kinds |= {c["record"][0] for c in rec["candidates"][:rec["consumed"]]}
    assert rm.KIND_SCALAR_RUIN in kinds and len(kinds) >= 2


def _check_records_one_by_one(oracle, d, o, leaf, r, order, seed, step_index, levels, list_desc=None):
    """A step whose union order the mirror does not restate: every record on its own, and the state after the pick."""
    gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 14)
    table = d.scalar_ruin_table(r)
    ctx = rm.Context(oracle, step_index, oracle.lib().sfo_step_seed(seed, step_index), order)
    mtable = leaf.open(ctx)
    assert table == rm.public_table(mtable)
    emitted = [(i, row) for i, row in enumerate(mtable) if row["emitted"]]
    ruin = [(rec, tuple(s)) for rec, s in zip(_t(gm), gs.tolist()) if rec[0] == rm.KIND_SCALAR_RUIN]
    assert [rec for rec, _ in ruin] == [(rm.KIND_SCALAR_RUIN, i, len(row["entities"]), row["entities"][0], 0, 0) for i, row in emitted[:len(ruin)]]  # a prefix, in order
    assert [s for _, s in ruin] == [row["score"] for _, row in emitted[:len(ruin)]]
    others = np.array([k != rm.KIND_SCALAR_RUIN for k in gm["kind"]], dtype=bool)
    if others.any():
        sc, dv = o.evaluate_moves(gm[others])
        assert (dv != 0).tolist() == ((gf[others] & 1) != 0).tolist()
        assert [tuple(row[:levels]) for row, ok in zip(sc.tolist(), dv) if ok] == [tuple(row) for row, ok in zip(gs[others].tolist(), dv) if ok]
    if gap:
        if int(gmv["kind"]) == rm.KIND_SCALAR_RUIN:
            leaf.commit(mtable[int(gmv["a"])])
        else:
            o.apply_move(gmv)
    assert d.working_values(0, 0, replica=r).tolist() == leaf.values()
    assert tuple(d.calculate_score()[r].tolist()) == leaf.score()
    if list_desc is not None:
        assert d.working_lists(list_desc, r) == o.get_lists(list_desc)
    assert (d.fresh_score() == d.calculate_score()).all()
    return len(ruin), int(others.sum())


def test_stratified_random_union(oracle):
    name = "colouring_ff"
    s = rc.SCRIPTS[name]
    d = _start(name, before=(1, 2), search=(rc.LA, rc.COUNT))  # the default root union: StratifiedRandom, equal weights
    o = rc.oracle_model(oracle, name)
    leaf = rc.leaf_of(oracle, name, o)
    seen = [0, 0]
    for step in range(6):
        a, b = _check_records_one_by_one(oracle, d, o, leaf, 0, s["order"], s["seed"], step, rc.LEVELS)
        seen = [seen[0] + a, seen[1] + b]
    assert seen[0] > 0 and seen[1] > 0


def test_mixed_job_shop_beside_a_list_change_leaf(oracle):
    import solverforge_amd as sfa
    from solverforge_amd.director import SelectorKind
    from test_gpu_mixed import _jobshop

    p = _jobshop(n_jobs=6, n_machines=4, seed=2)
    d = sfa.build_jobshop(p, n_replicas=2, bendable=False, leaves=())
    d.add_selector(SelectorKind.LIST_CHANGE, 1)
    d.add_scalar_ruin_selector(0, min_ruin_count=2, max_ruin_count=4, moves_per_step=6, recreate=rm.CHEAPEST_INSERTION, variable_name="machine_idx")
    d.configure(sfa.SolverConfig(acceptor=rc.LA, late_acceptance_size=5, forager=rc.COUNT, accepted_count_limit=6, random_ties=False, selection_order=3, random_seed=21))
    d.calculate_score()
    d.phase_start()
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=False)
    leaf = rm.RuinLeaf(oracle, o, len(p["job"]), len(p["sequences"]), 21, variable_name="machine_idx", min_ruin_count=2, max_ruin_count=4, moves_per_step=6,
                       recreate=rm.CHEAPEST_INSERTION)
    seen = [0, 0]
    for step in range(6):
        a, b = _check_records_one_by_one(oracle, d, o, leaf, 0, 3, 21, step, 2, list_desc=1)
        seen = [seen[0] + a, seen[1] + b]
    assert seen[0] > 0 and seen[1] > 0


@pytest.mark.parametrize("name", ["colouring_ci", "assignment_range", "balance_counts"])
def test_fused_runs_end_where_the_traced_run_did(oracle, name):
    recs, want, _ = _traced(oracle, name)
    n = rc.SCRIPTS[name]["steps"]
    _, search = rc.search_of(oracle, name)
    for _ in range(n):
        search.step()
    nxt = rm.public_table(search.step(dry_run=True)["table"])
    for mode in ("one_launch", "two_launches", "budget"):
        d = _start(name)
        if mode == "one_launch":
            d.solve_steps(n)
        elif mode == "two_launches":
            d.solve_steps(3)
            d.solve_steps(n - 3)
        else:
            d.solve_moves(n, 1 << 20)
        assert _snapshot(d) == want, mode
        assert (d.fresh_score() == d.calculate_score()).all()
        seed = oracle.lib().sfo_step_seed(rc.SCRIPTS[name]["seed"], n)
        d.open_cursor(n, seed, selection_order=rc.SCRIPTS[name]["order"])
        assert d.scalar_ruin_table(0) == nxt, mode  # the stream state, seen through the next step's table


def test_three_replicas_have_their_own_streams(oracle):
    name, R = "colouring_ci", 3
    tables = []
    for r in range(R):
        d = _start(name, n_replicas=R)
        o, search = rc.search_of(oracle, name, replica=r)
        for step in range(4):
            _check_step(d, search, r, (r, step))
        tables.append(d.scalar_ruin_table(r))
    assert tables[0] != tables[1] != tables[2] != tables[0]


def test_a_launch_of_several_residencies(oracle):
    from test_gpu_large_launch import _cus  # (asked in a child process: the pytest process stays torch-free)

    name, steps = "colouring_original", 6
    R = 2 * 32 * _cus() + 37
    d = _start(name, n_replicas=R)
    d.solve_steps(steps)
    assert (d.fresh_score() == d.calculate_score()).all()
    for r in np.linspace(0, R - 1, 16).astype(int).tolist():
        _, search = rc.search_of(oracle, name, replica=r)
        for _ in range(steps):
            search.step()
        assert _snapshot(d, r) == _mirror_snapshot(search), r


def test_open_cursor_is_a_dry_run(oracle):
    name = "colouring_ff"
    s = rc.SCRIPTS[name]
    d = _start(name)
    o, search = rc.search_of(oracle, name)
    for step in range(2):
        seed = oracle.lib().sfo_step_seed(s["seed"], step)
        gm, gs, gd = d.open_cursor(step, seed, selection_order=s["order"])
        rec = search.step(dry_run=True)
        assert d.scalar_ruin_table(0) == rm.public_table(rec["table"])
        assert _t(gm) == [c["record"] for c in rec["candidates"]] and [tuple(x) for x in gs.tolist()] == [c["score"] for c in rec["candidates"]] and gd.all()
        _check_step(d, search, 0, step)  # the traced step sees the same table: the dry run did not advance the stream


def test_validation(oracle):
    import solverforge_amd as sfa
    name = "colouring_ff"
    d = rc.device_model(name)
    for kw, code, msg in ((dict(min_ruin_count=0), "INVALID", "min_ruin_count"), (dict(min_ruin_count=3, max_ruin_count=2), "INVALID", "max_ruin_count"),
                          (dict(max_ruin_count=9), "UNSUPPORTED", "at most 8 entities"), (dict(moves_per_step=17), "UNSUPPORTED", "at most 16 moves"),
                          (dict(recreate=2), "INVALID", "recreate heuristic"), (dict(value_candidate_limit=-2), "INVALID", "value_candidate_limit"),
                          (dict(), "UNSUPPORTED", "one scalar ruin leaf per scalar variable")):
        with pytest.raises(sfa.SolverForgeError, match=code + ".*" + msg):
            d.add_scalar_ruin_selector(0, **kw)
    rc.configure(d, name)
    d.calculate_score()
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*frozen"):
        d.add_scalar_ruin_selector(0)
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*sf_phase_start first"):  # (every fused launch says so, with or without the leaf)
        d.solve_steps(1)
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*scalar ruin leaf.*sf_phase_start seeds its stream"):
        d.open_cursor(0, 0)  # sf_step_generate needs no started phase, the leaf's stream does
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.scalar_ruin_table(0)
    d.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*neither traced nor generated"):
        d.scalar_ruin_table(0)
    record = (rm.KIND_SCALAR_RUIN, 0, 2, 0, 0, 0)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*SF_MOVE_SCALAR_RUIN"):
        d.evaluate_moves(np.array([record], dtype=sfa.MOVE_DTYPE))
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*SF_MOVE_SCALAR_RUIN"):
        d.apply_move(record)
    import ctypes as C
    from solverforge_amd._lib import check, ptr

    edits, off = np.array([record], dtype=sfa.MOVE_DTYPE), np.array([0, 1], dtype=np.int64)
    scores, flags, consumed, selected = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.int32), C.c_int64(0), C.c_int64(-1)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*SF_MOVE_SCALAR_RUIN"):
        check(d._L.sf_step_decide_cursor(d._h, 0, ptr(edits), ptr(off), None, 1, ptr(scores), ptr(flags), C.byref(consumed), C.byref(selected)), d._h)
    # a forced engine, TabuSearch, Variable Neighborhood Descent
    d.set_engine(sfa.Engine.BLOCK)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*scalar ruin leaf.*generic engine only"):
        d.solve_steps(1)
    d.set_engine(0)
    d.configure_tabu()
    d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.TABU_SEARCH, late_acceptance_size=rc.LA_SIZE, forager=2, random_seed=1))
    d.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*tabu search.*ruin"):
        d.solve_steps(1)
    d.configure_vnd()
    d.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*variable neighborhood descent.*scalar ruin leaf"):
        d.solve_steps(1)
    # the join of the two planning classes; a dynamic nearby scalar slot
    from solverforge_amd.director import SelectorKind
    from test_gpu_mixed import _jobshop

    p = _jobshop(n_jobs=6, n_machines=4, seed=2)
    dj = sfa.build_jobshop(p, n_replicas=1, bendable=False, leaves=(), owner_match_level=1)
    dj.add_selector(SelectorKind.LIST_CHANGE, 1)
    dj.add_scalar_ruin_selector(0, variable_name="machine_idx")
    dj.configure(sfa.SolverConfig(random_seed=1))
    dj.calculate_score()
    dj.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*scalar ruin leaf.*join of the two planning classes"):
        dj.solve_steps(1)
    g = rc.problem(name)
    dn = sfa.build_graph_coloring(g, leaves=())
    dn.add_nearby_scalar_selector(SelectorKind.NEARBY_SCALAR_CHANGE, 0, [list(range(g["n_colors"]))] * g["n"], dynamic=True)
    dn.add_scalar_ruin_selector(0)
    dn.configure(sfa.SolverConfig(random_seed=1))
    dn.calculate_score()
    dn.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*scalar ruin leaf.*dynamic nearby scalar"):
        dn.solve_steps(1)


def test_the_way_back(oracle):
    """A context without the leaf takes its usual engine, and engine() is what it was for a scalar-only model."""
    import solverforge_amd as sfa

    g = rc.problem("colouring_ff")
    d0, d1 = sfa.build_graph_coloring(g), rc.device_model("colouring_ff")
    for d in (d0, d1):
        d.configure(sfa.SolverConfig(random_seed=3))
        d.calculate_score()
        d.phase_start()
        d.solve_steps(3)
    assert d0.engine() == d1.engine()
    assert d0.arith_flags()[1] is None and d0.arith_flags()[0]["scalar_value_bytes"] == 1  # the scalar engine, no generic launch
    assert d1.arith_flags()[1] is not None and d1.arith_flags()[0]["scalar_value_bytes"] == 0
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    o.configure(leaves=3, random_seed=3)
    o.phase_start()
    o.steps(3)
    assert (d0.working_values(0, 0) == o.get_vars(0, 0)).all()


def test_entities_past_65535(oracle):
    """One traced step on a sparse graph of 140,000 vertices (one-byte values in the LDS slice, the oracle's indexed join): more than
    half of the indices lie past 65,535, and the table's entities are full 32-bit words."""
    import solverforge_amd as sfa

    n, seed = 140_000, 23
    g = rc.graph(n, 150_000, 3, seed=31)
    d = sfa.build_graph_coloring(g, leaves=())
    d.add_scalar_ruin_selector(0, min_ruin_count=4, max_ruin_count=8, moves_per_step=16, recreate=rm.CHEAPEST_INSERTION)
    d.configure(sfa.SolverConfig(acceptor=rc.HC, forager=rc.BEST, random_ties=False, selection_order=rc.RANDOM, random_seed=seed))
    d.calculate_score()
    d.phase_start()
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"], indexed=True)
    leaf = rm.RuinLeaf(oracle, o, n, g["n_colors"], seed, min_ruin_count=4, max_ruin_count=8, moves_per_step=16, recreate=rm.CHEAPEST_INSERTION)
    search = rm.Search(oracle, o, leaf, seed, acceptor=rc.HC, forager=rc.BEST, order=rc.RANDOM)
    _, rec = _check_step(d, search, 0, "140,000 vertices")
    assert d.arith_flags()[1]["value_bytes"] == 1
    assert any(e > 65535 for row in rec["table"] for e in row["entities"]) and any(row["emitted"] for row in rec["table"])
