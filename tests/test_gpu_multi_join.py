"""GPU tests of scalar classes with several predicate joins (up to SF_MAX_PAIR_JOINS = 4 sf_constraint_add_pair_join programs / presets per
class, each on its own level and weight; stream/join_target.rs:28-110 scores any number of joins per class).

(1) Against the unchanged CPU oracle: one join of an oracle model split into two DISJOINT joins on the same level and weight has the oracle's
score in every state, so candidate streams, trial scores, fused trajectories and counters must equal the oracle's bit for bit.
(2) A timetable-shaped class with four joins on two levels against a brute-force count over all pairs."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _t4(moves):
    return np.stack([moves["kind"], moves["a"], moves["b"], moves["value"]], axis=1)


def _split_csr(off, adj, half):
    """The unordered pairs {u, v} of a CSR whose (u + v) % 2 == half, both directions kept (a pair never lands in both halves)."""
    n = len(off) - 1
    rows = [[int(v) for v in adj[off[u]:off[u + 1]] if (u + int(v)) % 2 == half] for u in range(n)]
    o = np.zeros(n + 1, dtype=np.asarray(off).dtype)
    o[1:] = np.cumsum([len(r) for r in rows])
    a = np.asarray([v for r in rows for v in r], dtype=np.asarray(adj).dtype)
    return o, a


def _sentinel_split(key, parity):
    """key where key % 2 == parity, a unique negative sentinel elsewhere: COL_EQ on it matches the pairs of `key` with that parity only."""
    key = np.asarray(key, dtype=np.int64)
    out = np.where(key % 2 == parity, key, -(np.arange(len(key)) + 1))
    return out.astype(np.int32)


# ---- (1) split joins against the oracle --------------------------------------------------------------------------------------------
def _graph_split(g, n_replicas, mixed):
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp, SelectorKind

    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=n_replicas)
    d.add_entity_class(0, g["n"])
    d.add_scalar_variable(0, 0, g["n_colors"], True, g["colors"])
    for f, half in ((20, 0), (21, 1)):
        o, a = _split_csr(g["adj_off"], g["adj"], half)
        d.add_fact_csr(f, o, a)
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    if mixed:  # one preset, one program
        d.add_constraint(ConstraintKind.CROSS_ADJACENT_EQUAL, 0, fact=20, level=0, weight=1)
    else:
        d.add_pair_join(0, [(PairOp.CSR_CONTAINS, 0, 20), (PairOp.VALUE_EQ, 1)], level=0, weight=1)
    d.add_pair_join(0, [(PairOp.CSR_CONTAINS, 0, 21), (PairOp.VALUE_EQ, 1)], level=0, weight=1)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    return d


def _graph(n=300, e=1500, k=6, seed=3):
    from solverforge_amd import datasets

    g = datasets.make_graph(n, e, k, seed=seed)
    r = datasets.stream(seed + 99, n)
    g["colors"] = (r % np.uint64(k + 1)).astype(np.int64) - 1
    return g


@pytest.mark.parametrize("acceptor", ["late", "anneal"])
@pytest.mark.parametrize("mixed", [False, True])
def test_graph_colouring_two_csr_halves(oracle, acceptor, mixed):
    import solverforge_amd as sfa

    g = _graph()
    R = 3
    d = _graph_split(g, R, mixed)
    bits = oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    d.configure(sfa.SolverConfig(random_seed=2))
    s = d.calculate_score()
    assert (s[0] == o.score()[:2]).all() and s[0][0] < 0
    gs, gc = d.evaluate_each()
    os_, oc = o.evaluate_each()
    assert len(gs) == 3 and (gs[0] == os_[0, :2]).all() and (gs[1] + gs[2] == os_[1, :2]).all() and gc[1] + gc[2] == oc[1] and gc[1] > 0 and gc[2] > 0
    for order in (0, 3):
        o.configure(leaves=bits, selection_order=order)
        gm, gsc, gd = d.open_cursor(7, 41, selection_order=order, cap=1 << 17)
        om = o.enumerate(0, 7, 41, order)
        assert len(gm) == len(om) > 0 and (_t4(gm) == _t4(om)).all()
        osc, od = o.evaluate_moves(om)
        assert (gd == od).all() and (gsc == osc[:, :2]).all()
    if acceptor == "late":
        d.configure(sfa.SolverConfig(random_seed=2))
    else:
        d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.SIMULATED_ANNEALING, forager=0, accepted_count_limit=1, random_seed=2))
        d.configure_annealing(mode=2, calibration_sample_size=40, seed=2)
    d.phase_start()
    d.solve_steps(40)
    d.solve_steps(20)
    for r in (0, R - 1):
        o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
        if acceptor == "late":
            o.configure(leaves=bits, random_seed=2 + r)
        else:
            o.configure(acceptor=1, forager=0, limit=1, leaves=bits, random_seed=2 + r)
            o.configure_annealing(mode=2, sample_size=40, seed=2 + r)
        o.phase_start()
        o.steps(60)
        assert (d.calculate_score()[r] == o.score()[:2]).all(), r
        assert (d.working_values(0, 0, r) == o.get_vars(0, 0)).all(), r
        assert d.stats(r)["moves_evaluated"] == o.stats()["moves_evaluated"], r
    assert (d.fresh_score() == d.calculate_score()).all()


def test_nqueens_as_two_programs(oracle):
    """{COL_NE} and {VALUE_EQ} / {COL_NE} and {VALUE_ABSDIFF_EQ_COL}: disjoint (a shared row is a row difference of 0, never the column
    difference of two distinct columns), two interpreted dense scans whose sum is the queens join."""
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp, SelectorKind
    import solverforge_amd as sfa

    n = 48
    rows = (np.arange(n) * 7 % (n + 1)).astype(np.int64) - 1
    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=1)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, n, True, rows)
    d.add_fact_column_i32(30, np.arange(n, dtype=np.int32))
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    d.add_pair_join(0, [(PairOp.COL_NE, 0, 30), (PairOp.VALUE_EQ, 1)], level=0, weight=1)
    d.add_pair_join(0, [(PairOp.COL_NE, 0, 30), (PairOp.VALUE_ABSDIFF_EQ_COL, 1, 30)], level=0, weight=1)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    o = oracle.Model.nqueens(rows)
    o.configure(leaves=oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, random_seed=3)
    d.configure(sfa.SolverConfig(random_seed=3))
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    gm, gs, gd = d.open_cursor(1, 5, selection_order=3, cap=1 << 16)
    om = o.enumerate(0, 1, 5, 3)
    assert (_t4(gm) == _t4(om)).all()
    os_, od = o.evaluate_moves(om)
    assert (gd == od).all() and (gs == os_[:, :2]).all()
    d.phase_start()
    o.phase_start()
    d.solve_steps(40)
    o.steps(40)
    assert (d.working_values(0, 0) == o.get_vars(0, 0)).all()
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()


def _shift_split(nurse, day, n_nurses, n_replicas, limit, w_streak, count_weight, target):
    """build_shift_schedule with its `one shift per nurse-day` join split by day parity (two sentinel columns)."""
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd.models import FACT_COLUMN, FACT_GROUP

    n = len(nurse)
    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=n_replicas)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, n_nurses, True, nurse)
    d.add_fact_column_i32(FACT_GROUP, np.asarray(day, dtype=np.int32))
    d.add_fact_column_i32(40, _sentinel_split(day, 0))
    d.add_fact_column_i32(41, _sentinel_split(day, 1))
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    d.add_constraint(ConstraintKind.CROSS_GROUP_EQUAL, 0, fact=40, level=0, weight=1)
    d.add_constraint(ConstraintKind.CROSS_GROUP_EQUAL, 0, fact=41, level=0, weight=1)
    d.add_constraint(ConstraintKind.RUNS_VALUE, 0, fact=FACT_GROUP, param=limit, level=1, weight=w_streak)
    d.add_fact_column_i32(FACT_COLUMN, np.ones(n, dtype=np.int32))
    d.add_constraint(ConstraintKind.COMPLEMENTED_VALUE_SUM, 0, fact=FACT_COLUMN, param=target, level=1, weight=count_weight)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    return d


def test_shift_schedule_split_join(oracle):
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    n_nurses, n_days, per_day = 6, 14, 3
    n = n_days * per_day
    day = np.repeat(np.arange(n_days), per_day).astype(np.int64)
    nurse = (datasets.stream(14, n) % np.uint64(n_nurses)).astype(np.int64)
    nurse[::7] = -1
    kw = dict(limit=2, w_streak=2, count_weight=1, target=5)
    d = _shift_split(nurse, day, n_nurses, 2, **kw)
    o = oracle.Model.shift_schedule(nurse, day, n_nurses, **kw)
    assert (d.calculate_score()[0] == o.score()[:2]).all()
    gs, gc = d.evaluate_each()
    os_, oc = o.evaluate_each()
    assert len(gs) == 5
    assert (gs[0] == os_[0, :2]).all() and (gs[1] + gs[2] == os_[1, :2]).all() and (gs[3:] == os_[2:, :2]).all()
    assert gc[0] == oc[0] and gc[1] + gc[2] == oc[1] and (gc[3:] == oc[2:]).all()
    bits = oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    for order in (0, 3):
        o.configure(leaves=bits, selection_order=order)
        gm, gsc, gd = d.open_cursor(4, 99, selection_order=order, cap=1 << 18)
        om = o.enumerate(0, 4, 99, order)
        assert len(gm) == len(om) > 0 and (_t4(gm) == _t4(om)).all()
        osc, od = o.evaluate_moves(om)
        assert (gd == od).all() and (gsc == osc[:, :2]).all()
        es, ed = d.evaluate_moves(om)  # sf_step_evaluate
        assert (ed == od).all() and (es == osc[:, :2]).all()
    o.configure(leaves=bits, selection_order=3)
    mv = o.enumerate(0, 2, 9, 3)
    sc, do = o.evaluate_moves(mv)
    mv = mv[(do != 0) & (mv["kind"] == 1)][3]
    o.apply_move(mv)
    d.apply_move(mv, replica=0)  # sf_apply
    d.apply_move(mv, replica=1)
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()
    o.configure(leaves=bits, random_seed=5, la_size=9, limit=30)
    d.configure(sfa.SolverConfig(random_seed=5, late_acceptance_size=9, accepted_count_limit=30))
    d.phase_start()
    o.phase_start()
    d.solve_steps(30)
    o.steps(30)
    assert (d.working_values(0, 0, 0) == o.get_vars(0, 0)).all()
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score() == d.calculate_score()).all()
    gst, ost = d.stats(0), o.stats()
    for k in ["step_count", "moves_evaluated", "moves_accepted", "moves_applied"]:
        assert gst[k] == ost[k], k


def test_jobshop_split_join_generic_engine(oracle):
    """The mixed job shop (scalar class + list class, generic engine) with `same job && same machine` split by job parity."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind
    from solverforge_amd.models import FACT_CUSTOMERS

    p = datasets.make_jobshop(10, 4)
    n, n_m = p["n_ops"], p["n_machines"]
    r = datasets.stream(5, 3 * n)
    p["machine_idx"] = (r[:n] % np.uint64(n_m + 1)).astype(np.int64) - 1
    seqs = [[] for _ in range(n_m)]
    for op in range(n):
        w = int(r[n + op] % np.uint64(n_m + 2))
        if w < n_m:
            seqs[w].append(op)
    p["sequences"] = seqs
    d = GpuScoreDirector(score_levels=3, hard_levels=2, n_replicas=2)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, n_m, True, p["machine_idx"])
    d.add_entity_class(1, n_m)
    d.add_list_variable(1, p["sequences"], element_capacity=n, element_id_bound=n)
    d.add_fact_column_i32(40, _sentinel_split(p["job"], 0))
    d.add_fact_column_i32(41, _sentinel_split(p["job"], 1))
    d.add_fact_column_u32(FACT_CUSTOMERS, np.arange(n, dtype=np.uint32))
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    d.add_constraint(ConstraintKind.NOT_EXISTS_FLATTENED, 1, fact=FACT_CUSTOMERS, level=1, weight=1)
    d.add_constraint(ConstraintKind.CROSS_GROUP_EQUAL, 0, fact=40, level=2, weight=1)
    d.add_constraint(ConstraintKind.CROSS_GROUP_EQUAL, 0, fact=41, level=2, weight=1)
    d.add_selector(SelectorKind.LIST_CHANGE, 1)
    d.add_selector(SelectorKind.LIST_SWAP, 1)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=True)
    bits = oracle.LEAF_LIST_CHANGE | oracle.LEAF_LIST_SWAP | oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    o.configure(leaves=bits, random_seed=4)
    d.configure(sfa.SolverConfig(random_seed=4))
    assert (d.calculate_score()[0] == o.score()[:3]).all()
    d.phase_start()
    o.phase_start()
    d.solve_steps(30)
    o.steps(30)
    assert (d.calculate_score()[0] == o.score()[:3]).all()
    assert (d.working_values(0, 0, 0) == o.get_vars(0, 0)).all()
    assert d.working_lists(1, 0) == o.get_lists(1)
    assert (d.fresh_score() == d.calculate_score()).all()


# ---- (2) four joins on two levels against brute force ------------------------------------------------------------------------------
def _holds(prog, cols, l, r, vl, vr):
    from solverforge_amd.director import PairOp as P

    clauses = {}
    for op, cl, fact, _fb, param in prog:
        if op == P.VALUE_EQ:
            h = vl == vr
        elif op == P.VALUE_ABSDIFF_LE:
            h = abs(vl - vr) <= param
        elif op == P.COL_EQ:
            h = cols[fact][l] == cols[fact][r]
        elif op == P.COL_LT:
            h = cols[fact][l] < cols[fact][r]
        else:
            raise AssertionError(op)
        clauses[cl] = clauses.get(cl, False) or bool(h)
    return all(clauses.values())


def _count(prog, cols, vals):
    n = len(vals)
    return sum(1 for l, r in itertools.combinations(range(n), 2) if vals[l] >= 0 and vals[r] >= 0 and _holds(prog, cols, l, r, int(vals[l]), int(vals[r])))


def _timetable(n=64, k=8, n_replicas=2, seed=11, joins=4):
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, PairOp as P, SelectorKind
    from solverforge_amd import datasets

    r = datasets.stream(seed, 5 * n)
    vals0 = (r[:n] % np.uint64(k + 1)).astype(np.int64) - 1
    cols = {50: (r[n:2 * n] % np.uint64(9)).astype(np.int32),       # teacher
            51: (r[2 * n:3 * n] % np.uint64(7)).astype(np.int32),   # student group
            52: (r[3 * n:4 * n] % np.uint64(6)).astype(np.int32),   # room
            53: (r[4 * n:5 * n] % np.uint64(40)).astype(np.int32)}  # a soft key
    progs = [([(P.COL_EQ, 0, 50, -1, 0), (P.VALUE_EQ, 1, -1, -1, 0)], 0, 1),
             ([(P.COL_EQ, 0, 51, -1, 0), (P.VALUE_EQ, 1, -1, -1, 0)], 0, 1),
             ([(P.COL_EQ, 0, 52, -1, 0), (P.VALUE_EQ, 1, -1, -1, 0)], 0, 1),
             ([(P.COL_LT, 0, 53, -1, 0), (P.VALUE_ABSDIFF_LE, 1, -1, -1, 1)], 1, 3)][:joins]
    d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=n_replicas)
    d.add_entity_class(0, n)
    d.add_scalar_variable(0, 0, k, True, vals0)
    for f, c in cols.items():
        d.add_fact_column_i32(f, c)
    d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
    for prog, level, weight in progs:
        d.add_pair_join(0, prog, level=level, weight=weight)
    d.add_selector(SelectorKind.SCALAR_CHANGE, 0)
    d.add_selector(SelectorKind.SCALAR_SWAP, 0)

    def expect(vals):
        s = [-int((vals < 0).sum()), 0]
        for prog, level, weight in progs:
            s[level] -= weight * _count(prog, cols, vals)
        return s

    return d, vals0, progs, cols, expect


@pytest.mark.parametrize("interpret", ["0", "1"])
def test_timetable_four_joins_against_brute_force(monkeypatch, interpret):
    """Three hard conflicts behind COL_EQ partner indices (specialised loops, or all interpreted with SF_AMD_IR_INTERPRET=1) beside a soft
    dense join (always interpreted): the two kinds mixed in one class."""
    import solverforge_amd as sfa

    monkeypatch.setenv("SF_AMD_IR_INTERPRET", interpret)
    d, vals0, progs, cols, expect = _timetable()
    d.configure(sfa.SolverConfig(random_seed=6))
    s = d.calculate_score()
    assert s[0].tolist() == expect(vals0) and s[0][0] < 0 and s[0][1] < 0
    gs, gc = d.evaluate_each()
    assert len(gs) == 5
    for i, (prog, level, weight) in enumerate(progs):
        c = _count(prog, cols, vals0)
        assert gc[i + 1] == c and gs[i + 1][level] == -weight * c and gs[i + 1][1 - level] == 0, i
    gm, gsc, gd = d.open_cursor(3, 17, selection_order=3, cap=1 << 15)
    assert len(gm) > 100
    for i in range(0, len(gm), 7):
        mv = gm[i]
        v = vals0.copy()
        if mv["kind"] == 0:
            v[mv["a"]] = mv["value"]
        else:
            v[mv["a"]], v[mv["b"]] = vals0[mv["b"]], vals0[mv["a"]]
        if gd[i]:
            assert gsc[i].tolist() == expect(v), (i, mv)
    # host-driven paths: compound candidates (sf_step_evaluate_compound), apply_candidate, step_decide (hill climbing)
    rng = np.random.default_rng(4)
    n, k = len(vals0), 8
    cands = [[(int(e), int(rng.integers(-1, k))) for e in rng.choice(n, size=int(rng.integers(2, 4)), replace=False)] for _ in range(40)]
    cs_, cd = d.evaluate_candidates(cands)
    for i, c in enumerate(cands):
        if cd[i]:
            v = vals0.copy()
            for e, to in c:
                v[e] = to
            assert cs_[i].tolist() == expect(v), i
    d.apply_candidate(cands[5])
    v = vals0.copy()
    for e, to in cands[5]:
        v[e] = to
    assert d.calculate_score()[0].tolist() == expect(v) and d.fresh_score()[0].tolist() == expect(v)
    assert (np.asarray(d.working_values(0, 0, 0), dtype=np.int64) == v).all()
    before = tuple(d.calculate_score()[0])
    d.configure(sfa.SolverConfig(acceptor=sfa.Acceptor.HILL_CLIMBING, random_seed=6))
    _kept, ts, _flags, sel = d.step_decide(cands)
    v2 = np.asarray(d.working_values(0, 0, 0), dtype=np.int64)
    after = d.calculate_score()[0]
    assert after.tolist() == expect(v2) and (d.fresh_score()[0] == after).all()
    if any(tuple(t) > before for t in ts):
        assert sel >= 0 and tuple(after) > before
    # fused steps on both replicas
    d.configure(sfa.SolverConfig(random_seed=6))
    d.phase_start()
    d.solve_steps(25)
    sc = d.calculate_score()
    assert (d.fresh_score() == sc).all()
    for rep in range(2):
        assert sc[rep].tolist() == expect(np.asarray(d.working_values(0, 0, rep), dtype=np.int64)), rep


def test_limits():
    import solverforge_amd as sfa
    from solverforge_amd.director import PairOp as P

    d, vals0, _progs, _cols, expect = _timetable(n=24, joins=4)
    assert d.calculate_score()[0].tolist() == expect(vals0)  # four joins are accepted
    d, *_ = _timetable(n=24, joins=4)
    d.add_pair_join(0, [(P.COL_EQ, 0, 50), (P.VALUE_NE, 1)], level=0, weight=1)
    with pytest.raises(sfa.SolverForgeError, match="4"):
        d.calculate_score()  # a fifth is refused at initialize
    d, *_ = _timetable(n=24, joins=1)
    d.add_pair_join(0, [(P.COL_EQ, 0, 99), (P.VALUE_EQ, 1)], level=0, weight=1)  # a second program over a fact that does not exist
    with pytest.raises(sfa.SolverForgeError):
        d.calculate_score()
    d, vals0, progs, cols, expect = _timetable(n=24, joins=1)  # one join: one row, the class's own join fields
    assert d.calculate_score()[0].tolist() == expect(vals0)
    gs, gc = d.evaluate_each()
    assert len(gs) == 2 and gc[1] == _count(progs[0][0], cols, vals0) and gs[1].tolist() == [-gc[1], 0]
