"""GPU parity of sf_construct_scalar (csrc/sf_scalar_construct.hip), through the C ABI and bit-exact: values of every replica, committed
score == fresh score == expected score, counter deltas.  FirstFit / PreserveUnassigned is compared with the unchanged oracle's
construct_first_fit; every other heuristic x obligation, the value-candidate limit and a required variable with the mirror
(tests/scalar_construction_mirror.py), which tests/test_scalar_construction_mirror.py pins to the oracle and to the reference's literals."""
import ctypes as C

import numpy as np
import pytest

import scalar_construction_cases as cases
import scalar_construction_mirror as mirror

pytestmark = pytest.mark.gpu

ORACLE_COUNTERS = ("moves_evaluated", "score_calculations")  # what construct_first_fit records
MIRROR_COUNTERS = ("step_count", "moves_generated", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations", "moves_not_doable")


def _stats(d, r):
    import solverforge_amd as sfa

    try:
        return d.stats(r)
    except sfa.SolverForgeError as err:  # no phase has run on this context yet: the counters do not exist, i.e. they are all zero
        if "bad sf_get_stats" not in str(err):
            raise
        return {k: 0 for k in MIRROR_COUNTERS}


def _construct(d, R, **kw):
    """calculate_score (initialize), the call, and per replica (values, committed score, fresh score, counter deltas)."""
    d.calculate_score()
    before = [_stats(d, r) for r in range(R)]
    out = d.construct_scalar(0, 0, **kw)
    committed, fresh = d.calculate_score(), d.fresh_score()
    assert (out == committed).all()
    res = []
    for r in range(R):
        after = d.stats(r)
        res.append((d.working_values(0, 0, r), committed[r], fresh[r], {k: after[k] - before[r][k] for k in MIRROR_COUNTERS}))
    return res


def _same(res, values, score, counters, keys, what=""):
    vals, committed, fresh, delta = res
    L = len(committed)
    assert (vals == values).all(), (what, vals, values)
    assert (committed == score[:L]).all() and (fresh == score[:L]).all(), (what, committed, fresh, score)
    for k in keys:
        assert delta[k] == counters[k], (what, k, delta, counters)


def _mirror(oracle, case, heuristic, **kw):
    m = case.oracle(oracle)
    st = mirror.construct(m, heuristic, n_values=case.n_values, value_lists=case.value_lists, **kw)
    return m, st


# ---- FirstFit / PreserveUnassigned against the oracle itself ----------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(11))
def test_first_fit_equals_the_oracle(oracle, idx):
    case = ([c[0] for c in cases.first_fit_inputs()] + cases.other_first_fit_cases())[idx]
    o = case.oracle(oracle)
    o.construct_first_fit()
    assert (o.get_vars(0, 0) >= 0).any() and o.stats()["score_calculations"] > 0
    R = 2
    res = _construct(case.gpu(R), R)
    for r in range(R):
        _same(res[r], o.get_vars(0, 0), o.score(), o.stats(), ORACLE_COUNTERS, (case.name, r))
        assert res[r][3]["step_count"] == case.n and res[r][3]["moves_accepted"] == int((o.get_vars(0, 0) >= 0).sum())


def test_first_fit_on_the_interpreted_join_equals_the_oracle(oracle):
    case = cases.graph(70, 260, 4, 6, pair_ir=True)
    o = case.oracle(oracle)
    o.construct_first_fit()
    _same(_construct(case.gpu(1), 1)[0], o.get_vars(0, 0), o.score(), o.stats(), ORACLE_COUNTERS)


# ---- every other heuristic x obligation against the mirror ------------------------------------------------------------------------------
@pytest.mark.parametrize("obligation", [mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS])
@pytest.mark.parametrize("heuristic", mirror.HEURISTICS)
def test_heuristics_equal_the_mirror(oracle, heuristic, obligation):
    for case in (cases.graph(40, 150, 5, 4), cases.balance(), cases.assignment()):
        ek, vk = cases.keys(case.n, 4, 21), cases.keys(case.n_values, 3, 22)  # keys with ties
        m, st = _mirror(oracle, case, heuristic, obligation=obligation, entity_order_keys=ek, value_order_keys=vk)
        res = _construct(case.gpu(2), 2, heuristic=heuristic, obligation=obligation, entity_order_keys=ek, value_order_keys=vk)
        for r in range(2):
            _same(res[r], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, (case.name, heuristic, obligation, r))


@pytest.mark.parametrize("heuristic", mirror.LIVE_REFRESH)
def test_live_refresh_assigns_kept_entities_on_a_retry(oracle, heuristic):
    case = cases.retry_assignment()
    kw = dict(entity_order_keys=cases.RETRY_ENTITY_KEYS, value_order_keys=cases.retry_value_keys(heuristic))
    m, st = _mirror(oracle, case, heuristic, **kw)
    assert st["kept"] >= 1 and st["assigned_on_retry"] >= 1 and st["step_count"] > case.n
    _same(_construct(case.gpu(1), 1, heuristic=heuristic, **kw)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, heuristic)


def test_kept_list_longer_than_a_chunk_loses_entities_from_its_middle(oracle):
    """120 kept entities when the first assignment comes; every later assignment leaves the list from its head or its middle and the tail
    moves down across 64-lane chunks (tests/test_scalar_construction_mirror.py asserts that shape on the mirror)."""
    case = cases.long_retry_assignment()
    for heuristic in (mirror.ALLOCATE_ENTITY_FROM_QUEUE, mirror.FIRST_FIT_DECREASING):
        ek = np.zeros(case.n, dtype=np.int64) if heuristic == mirror.ALLOCATE_ENTITY_FROM_QUEUE else -np.arange(case.n, dtype=np.int64)  # both: index order
        m, st = _mirror(oracle, case, heuristic, entity_order_keys=ek)
        assert st["assigned_on_retry"] > 64
        _same(_construct(case.gpu(1), 1, heuristic=heuristic, entity_order_keys=ek)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, heuristic)


@pytest.mark.parametrize("heuristic", [mirror.FIRST_FIT, mirror.CHEAPEST_INSERTION, mirror.FIRST_FIT_DECREASING, mirror.STRONGEST_FIT])
def test_four_join_timetable_equals_the_mirror_over_brute_force(oracle, heuristic):
    """Three hard COL_EQ joins and one soft interpreted join of weight 3 on the second level, as in test_gpu_multi_join.py; the mirror runs
    over a brute-force count of all pairs."""
    case = cases.timetable()
    for obligation in (mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS):
        kw = dict(obligation=obligation, entity_order_keys=cases.keys(case.n, 4, 21), value_order_keys=cases.keys(case.n_values, 3, 22))
        m, st = _mirror(oracle, case, heuristic, **kw)
        _same(_construct(case.gpu(1), 1, heuristic=heuristic, **kw)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, (heuristic, obligation))


def test_live_refresh_on_a_graph_that_stays_partly_unassigned(oracle):
    """46 of 120 vertices keep current, and every assignment reopens the kept ones: the long retry lists."""
    case = cases.graph(120, 700, 3, 1)
    ek = cases.keys(case.n, 5, 8)
    for heuristic, vk in ((mirror.FIRST_FIT_DECREASING, None), (mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, [2, 0, 1]), (mirror.STRONGEST_FIT_DECREASING, [1, 3, 3])):
        m, st = _mirror(oracle, case, heuristic, entity_order_keys=ek, value_order_keys=vk)
        assert st["kept"] > case.n
        _same(_construct(case.gpu(1), 1, heuristic=heuristic, entity_order_keys=ek, value_order_keys=vk)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, heuristic)


# ---- value lists, the candidate limit, a required variable -------------------------------------------------------------------------------
def test_ragged_value_lists(oracle):
    case = cases.graph(40, 150, 5, 4, value_lists=cases.ragged_lists(40, 5))
    assert case.value_lists[2] == [] and len(case.value_lists[5]) == 1
    o = case.oracle(oracle)
    o.construct_first_fit()
    res = _construct(case.gpu(1), 1)[0]
    _same(res, o.get_vars(0, 0), o.score(), o.stats(), ORACLE_COUNTERS)
    assert res[0][2] == -1 and res[3]["step_count"] == 39  # the entity without values is no placement
    vk = [1, 0, 1, 0, 2]
    for heuristic in (mirror.CHEAPEST_INSERTION, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, mirror.WEAKEST_FIT, mirror.STRONGEST_FIT_DECREASING):
        for limit in (0, 2):
            kw = dict(value_candidate_limit=limit, entity_order_keys=cases.keys(40, 3, 2), value_order_keys=vk)
            m, st = _mirror(oracle, case, heuristic, **kw)
            _same(_construct(case.gpu(1), 1, heuristic=heuristic, **kw)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, (heuristic, limit))


def test_value_lists_that_are_all_empty_place_nothing(oracle):
    """No entity has a candidate: no placement, no counter moves -- also under AllocateToValueFromQueue, whose sorted copy of the lists is empty."""
    case = cases.graph(40, 150, 5, 4, value_lists=[[] for _ in range(40)])
    for heuristic in (mirror.FIRST_FIT, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE):
        m, st = _mirror(oracle, case, heuristic, value_order_keys=[1, 0, 1, 0, 2])
        assert st["step_count"] == 0 and (m.get_vars(0, 0) < 0).all()
        _same(_construct(case.gpu(1), 1, heuristic=heuristic, value_order_keys=[1, 0, 1, 0, 2])[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, heuristic)


@pytest.mark.parametrize("limit", [1, 3, 9])  # one, below the 7 values, above them
def test_value_candidate_limit(oracle, limit):
    case = cases.assignment()
    vk = [5, 4, 3, 2, 1, 0, 0]
    for heuristic in (mirror.FIRST_FIT, mirror.CHEAPEST_INSERTION, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, mirror.STRONGEST_FIT):
        for obligation in (mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS):
            kw = dict(obligation=obligation, value_candidate_limit=limit, value_order_keys=vk)
            m, st = _mirror(oracle, case, heuristic, **kw)
            assert m.get_vars(0, 0).max() < min(limit, 7)  # the cut comes before the value order
            _same(_construct(case.gpu(1), 1, heuristic=heuristic, **kw)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, (heuristic, obligation))


@pytest.mark.parametrize("heuristic", [mirror.FIRST_FIT, mirror.CHEAPEST_INSERTION, mirror.WEAKEST_FIT_DECREASING, mirror.ALLOCATE_ENTITY_FROM_QUEUE])
def test_required_variable_from_an_unassigned_start(oracle, heuristic):
    case = cases.graph(40, 150, 3, 4)
    kw = dict(entity_order_keys=cases.keys(40, 4, 21), value_order_keys=[1, 0, 1])
    m, st = _mirror(oracle, case, heuristic, allows_unassigned=False, **kw)
    assert (m.get_vars(0, 0) >= 0).all() and m.score()[0] < 0  # everything is assigned, conflicts and all
    _same(_construct(case.gpu(1, allows_unassigned=False), 1, heuristic=heuristic, **kw)[0], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS)


# ---- replicas that have diverged ---------------------------------------------------------------------------------------------------------
def test_divergent_replicas_each_equal_their_own_oracle(oracle):
    """Five replicas (a four-wave workgroup would not be full): different apply_move prefixes, one untouched, one fully assigned (a no-op)."""
    case = cases.graph(40, 150, 5, 4)
    R = 5
    d = case.gpu(R)
    d.calculate_score()
    starts = [np.full(case.n, -1, dtype=np.int64) for _ in range(R)]
    for r, entities in ((1, [39, 3, 17]), (2, list(range(0, 40, 2))), (3, [5])):
        for e in entities:
            starts[r][e] = (e * 7 + r) % 5
    starts[4] = (np.arange(case.n) * 3) % 5  # every vertex holds a colour, conflicts and all
    for r in range(R):
        for e in np.flatnonzero(starts[r] >= 0):
            d.apply_move((0, int(e), 0, 0, 0, int(starts[r][e])), replica=r)
    res = _construct(d, R)
    for r in range(R):
        o = case.oracle(oracle, start=starts[r])
        base = o.stats()
        o.construct_first_fit()
        delta = {k: o.stats()[k] - base[k] for k in ORACLE_COUNTERS}
        _same(res[r], o.get_vars(0, 0), o.score(), delta, ORACLE_COUNTERS, r)
    assert all(v == 0 for v in res[4][3].values())


# ---- hand-over to the search engine, a second call -----------------------------------------------------------------------------------------
def _t(m):
    return np.stack([m["kind"], m["a"], m["b"], m["value"]], axis=1)


@pytest.mark.parametrize("which", ["graph", "clique16"])
def test_local_search_continues_from_the_constructed_state(oracle, which):
    import solverforge_amd as sfa

    case = cases.graph(120, 700, 3, 1) if which == "graph" else cases.clique(130, 140)  # clique: 16-bit values in the search engine
    bits = oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP
    d = case.gpu(1)
    d.configure(sfa.SolverConfig(random_seed=9))
    _construct(d, 1)
    o = case.oracle(oracle)
    o.construct_first_fit()
    o.configure(leaves=bits, random_seed=9)
    d.phase_start()
    o.phase_start()
    gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 17)
    om, os_, of, oap, omv = o.step_traced()
    assert len(gm) == len(om) and (_t(gm) == _t(om)).all() and (gf == of).all() and (gs == os_[:, :2]).all() and gap == oap
    R = 2
    d = case.gpu(R)
    d.configure(sfa.SolverConfig(random_seed=9))
    _construct(d, R)
    d.phase_start()  # (the phase's counters start at zero: sf_phase_start clears them)
    d.solve_steps(12)
    for r in range(R):
        o = case.oracle(oracle)
        o.construct_first_fit()
        ob = o.stats()
        o.configure(leaves=bits, random_seed=9 + r)
        o.phase_start()
        o.steps(12)
        assert (d.working_values(0, 0, r) == o.get_vars(0, 0)).all(), r
        assert (d.calculate_score()[r] == o.score()[:2]).all() and (d.fresh_score()[r] == o.score()[:2]).all(), r
        assert d.stats(r)["moves_evaluated"] == o.stats()["moves_evaluated"] - ob["moves_evaluated"] > 0, r


def test_second_call_changes_nothing(oracle):
    """On a constructed model the placements that kept current are placed again (they are counted: steps, pulled candidates, trials) and keep
    again; nothing is accepted or applied, no value and no score moves."""
    case = cases.graph(120, 700, 3, 1)
    m, st1 = _mirror(oracle, case, mirror.FIRST_FIT)
    st2 = mirror.construct(m, mirror.FIRST_FIT, n_values=case.n_values)
    assert st2["moves_accepted"] == 0 and st2["step_count"] == 46 == st2["kept"] and st2["score_calculations"] == 46 * 3
    d = case.gpu(1)
    first = _construct(d, 1)[0]
    second = _construct(d, 1)[0]
    _same(second, first[0], m.score(), st2, MIRROR_COUNTERS)


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
def test_validation(oracle):
    import solverforge_amd as sfa
    from solverforge_amd import _lib

    case = cases.graph(40, 150, 5, 4)
    d = case.gpu(1)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):  # before sf_initialize
        d.construct_scalar(0, 0)
    d.calculate_score()
    ek, vk = np.zeros(40, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for bad in (dict(descriptor_index=1), dict(variable_index=1), dict(heuristic=9), dict(heuristic=-1), dict(obligation=2), dict(value_candidate_limit=-1)):
        with pytest.raises(sfa.SolverForgeError, match="INVALID"):
            d.construct_scalar(**bad)
    for h in mirror.NEEDS_ENTITY_KEYS:
        with pytest.raises(sfa.SolverForgeError, match="INVALID.*entity_order_keys"):
            d.construct_scalar(heuristic=h, value_order_keys=vk)
    for h in mirror.NEEDS_VALUE_KEYS:
        with pytest.raises(sfa.SolverForgeError, match="INVALID.*value_order_keys"):
            d.construct_scalar(heuristic=h, entity_order_keys=ek)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):  # one key per row / per value
        d.construct_scalar(heuristic=mirror.FIRST_FIT_DECREASING, entity_order_keys=ek[:-1])
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.construct_scalar(heuristic=mirror.WEAKEST_FIT, value_order_keys=vk[:-1])
    L = _lib.load()
    out = np.zeros((1, 2), dtype=np.int64)
    per_entity = _lib.ScalarConstructionConfigStruct(mirror.WEAKEST_FIT, 0, 0, 1)  # value keys that depend on the entity
    assert _lib.ERRORS[L.sf_construct_scalar(d._h, 0, 0, C.byref(per_entity), None, _lib.ptr(np.zeros(200, dtype=np.int64)), _lib.ptr(out))] == "SF_ERR_UNSUPPORTED"
    assert _lib.ERRORS[L.sf_construct_scalar(d._h, 0, 0, C.byref(_lib.ScalarConstructionConfigStruct(0, 0, 0, 2)), None, None, _lib.ptr(out))] == "SF_ERR_INVALID"
    assert _lib.ERRORS[L.sf_construct_scalar(d._h, 0, 0, None, None, None, _lib.ptr(out))] == "SF_ERR_INVALID"
    assert L.sf_construct_scalar(d._h, 0, 0, C.byref(_lib.ScalarConstructionConfigStruct(0, 0, 0, 0)), None, None, None) == 0  # out_scores may be NULL
    assert (d.working_values(0, 0) >= 0).any()
    # a list-only model has no scalar variable
    from solverforge_amd import datasets

    p = datasets.make_cvrp(12, 2, 55, seed=1)
    dl = sfa.build_cvrp(p, n_replicas=1)
    dl.calculate_score()
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        dl.construct_scalar(0, 0)


def test_the_join_of_the_two_planning_classes_is_refused():
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    d = sfa.build_jobshop(datasets.make_jobshop(3, 2), n_replicas=1, owner_match_level=1)
    d.calculate_score()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*two planning classes"):
        d.construct_scalar(0, 0)
