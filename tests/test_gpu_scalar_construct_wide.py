"""GPU parity of sf_construct_scalar (csrc/sf_scalar_construct.hip) where one 64-lane chunk is not enough, bit-exact like its sibling
tests/test_gpu_scalar_construct.py (whose _construct / _same / _mirror it uses):

  A. placements of 130 candidates (two full chunks and a tail of two): the best-fit carry across chunks and the keep-current test after the
     last one, the strength foragers' extreme in every chunk and on the sentinel of the invalid lanes, the value order of
     AllocateToValueFromQueue and the value-candidate limit around the chunk boundaries, first fit over value lists longer than a chunk,
     live refresh through a row of a later chunk;
  B. per-value tables of 65 to 130 values in LDS (balance with every grouped form, assignment with the exists node, the shift models
     whose runs table starts at the ALIGNED end of the count table), constructed values at indices >= 64;
  C. construction at a launch of several residencies whose replicas have diverged (a short fused search seeded random_seed + r);
  D. the LDS gate of the table models: the last admitted and the first refused value count, and both sides of 64 KiB of dynamic LDS.

FirstFit / PreserveUnassigned is compared with the oracle's construct_first_fit, everything else with the mirror over the oracle's
evaluate_moves / apply_move; tests/test_scalar_construction_mirror.py asserts on the CPU that every case has the shape it claims.

Not covered, because no input reaches it: every candidate of an unassigned entity is doable (a Change to a value the entity does not hold
is always doable), so the first-fit branch without a baseline always takes ordinal 0 and moves_not_doable stays 0."""
import time

import numpy as np
import pytest

import scalar_construction_cases as cases
import scalar_construction_mirror as mirror
from test_gpu_scalar_construct import MIRROR_COUNTERS, ORACLE_COUNTERS, _construct, _mirror, _same

pytestmark = pytest.mark.gpu

BOTH = (mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS)
STRENGTH = (mirror.WEAKEST_FIT, mirror.WEAKEST_FIT_DECREASING, mirror.STRONGEST_FIT, mirror.STRONGEST_FIT_DECREASING)
LIMITS = (63, 64, 65, 129, 131)


def _gpu_equals_mirror(oracle, case, heuristic, what, R=1, **kw):
    m, st = _mirror(oracle, case, heuristic, **kw)
    res = _construct(case.gpu(R), R, heuristic=heuristic, **kw)
    for r in range(R):
        _same(res[r], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, (case.name, heuristic, what, r))
    return m, st


def _gpu_equals_first_fit(oracle, case, R=1):
    o = case.oracle(oracle)
    o.construct_first_fit()
    res = _construct(case.gpu(R), R)
    for r in range(R):
        _same(res[r], o.get_vars(0, 0), o.score(), o.stats(), ORACLE_COUNTERS, (case.name, r))
    return o


# ---- A. foragers across chunk boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obligation", BOTH)
@pytest.mark.parametrize("ex_level", [-1, 0])
def test_best_fit_carries_its_best_across_chunks(oracle, ex_level, obligation):
    case = cases.best_fit_assignment(ex_level=ex_level)
    m, st = _gpu_equals_mirror(oracle, case, mirror.CHEAPEST_INSERTION, obligation, R=2, obligation=obligation)
    if ex_level < 0:
        assert m.get_vars(0, 0)[:10].tolist() == cases.BEST_FIT_VALUES and st["score_calculations"] == 3120
    elif obligation == mirror.PRESERVE_UNASSIGNED:
        assert st["kept"] >= 1 and st["candidates"][0] == 130  # the baseline beats all 130 trials


@pytest.mark.parametrize("heuristic", STRENGTH)
def test_strength_extreme_in_every_chunk(oracle, heuristic):
    case = cases.wide_assignment()
    ek = cases.keys(case.n, 4, 21)
    for name, (vk, limit, want) in cases.strength_keys(heuristic in (mirror.WEAKEST_FIT, mirror.WEAKEST_FIT_DECREASING)).items():
        for obligation in BOTH:
            m, _ = _gpu_equals_mirror(oracle, case, heuristic, (name, obligation), obligation=obligation, value_candidate_limit=limit,
                                      entity_order_keys=ek, value_order_keys=vk)
            assert (m.get_vars(0, 0) == want).all(), name


@pytest.mark.parametrize("heuristic", STRENGTH + (mirror.ALLOCATE_TO_VALUE_FROM_QUEUE,))
def test_value_lists_of_every_length_around_the_chunks(oracle, heuristic):
    case = cases.wide_assignment(value_lists=cases.wide_lists(24))
    for obligation in BOTH:
        for limit in (0,) + (LIMITS if heuristic == mirror.ALLOCATE_TO_VALUE_FROM_QUEUE else (64,)):
            _gpu_equals_mirror(oracle, case, heuristic, (obligation, limit), obligation=obligation, value_candidate_limit=limit,
                               entity_order_keys=cases.keys(case.n, 4, 21), value_order_keys=cases.wide_list_keys())


@pytest.mark.parametrize("form", ["range", "lists"])
def test_value_queue_past_a_chunk_and_the_cut_before_the_sort(oracle, form):
    """A clique of 100 with 130 colours: entity i walks the sorted order past the colours that are taken, so the order is read beyond its
    first 64 entries; nothing beyond the cut is ever taken."""
    case = cases.wide_clique(100, value_lists=cases.wide_lists(100) if form == "lists" else None)
    vk = cases.keys(cases.WIDE, 7, 71)  # keys with ties
    for limit in (0,) + LIMITS:
        for obligation in BOTH:
            m, _ = _gpu_equals_mirror(oracle, case, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, (limit, obligation), obligation=obligation,
                                      value_candidate_limit=limit, value_order_keys=vk)
            vals = m.get_vars(0, 0)
            ordinals = [case.value_lists[e].index(int(v)) if case.value_lists is not None else int(v) for e, v in enumerate(vals) if v >= 0]
            assert all(k < (limit or 131) for k in ordinals)
    case = cases.wide_assignment()  # and on the table model, range form
    for limit in LIMITS:
        _gpu_equals_mirror(oracle, case, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, limit, value_candidate_limit=limit, value_order_keys=vk)


@pytest.mark.parametrize("n,k,hits", [(70, 80, cases.ROTATED_HITS_70), (130, 140, cases.ROTATED_HITS_130)])
def test_first_fit_over_value_lists_longer_than_a_chunk(oracle, n, k, hits):
    case = cases.rotated_clique(n, k, hits)
    o = _gpu_equals_first_fit(oracle, case, R=2)
    assert o.get_vars(0, 0).tolist() == list(range(n))
    _gpu_equals_mirror(oracle, case, mirror.FIRST_FIT_DECREASING, "decreasing", entity_order_keys=cases.keys(n, 5, 8))


@pytest.mark.parametrize("heuristic", mirror.LIVE_REFRESH)
def test_live_refresh_through_a_row_of_a_later_chunk(oracle, heuristic):
    case = cases.wide_retry_assignment()
    _, st = _gpu_equals_mirror(oracle, case, heuristic, "retry", entity_order_keys=cases.RETRY_ENTITY_KEYS,
                               value_order_keys=cases.wide_retry_value_keys(heuristic))
    assert st["kept"] >= 1 and st["assigned_on_retry"] >= 1 and st["step_count"] > case.n


# ---- B. tables wider than the wave ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.wide_table_models()))
def test_tables_wider_than_the_wave(oracle, name):
    make = cases.wide_table_models()[name]
    case = make(None)
    ek = cases.keys(case.n, 4, 21)
    for heuristic in (mirror.FIRST_FIT, mirror.CHEAPEST_INSERTION, mirror.STRONGEST_FIT_DECREASING, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE):
        vk = cases.table_keys(case.n_values, least=heuristic == mirror.ALLOCATE_TO_VALUE_FROM_QUEUE)  # keys with ties, the extreme at values >= 64
        for obligation in BOTH:
            _gpu_equals_mirror(oracle, case, heuristic, obligation, R=2, obligation=obligation, entity_order_keys=ek, value_order_keys=vk)
    _gpu_equals_first_fit(oracle, case)
    listed = make(cases.rotated_lists(case.n, case.n_values))
    o = _gpu_equals_first_fit(oracle, listed, R=2)
    assert o.get_vars(0, 0).max() >= 64
    _gpu_equals_mirror(oracle, listed, mirror.FIRST_FIT, "listed", obligation=mirror.ASSIGN_WHEN_CANDIDATE_EXISTS)


# ---- C. at size: more than two residencies, diverged replicas ----------------------------------------------------------------------------
N_SAMPLE = 48


def _searched(case, R, seed):
    import solverforge_amd as sfa

    d = case.gpu(R)
    d.configure(sfa.SolverConfig(random_seed=seed))
    d.calculate_score()
    d.phase_start()
    d.solve_steps(cases.AT_SIZE_SEARCH_STEPS)
    return d


def _all_values(d, R):
    return np.stack([d.working_values(0, 0, r) for r in range(R)])


@pytest.mark.parametrize("heuristic", [mirror.FIRST_FIT, mirror.FIRST_FIT_DECREASING, mirror.ALLOCATE_ENTITY_FROM_QUEUE])
def test_construction_at_size_from_diverged_replicas(oracle, heuristic):
    """R = 2 * 32 * CUs + 37 replicas, each all-unassigned and then moved by 18 steps of the fused scalar search seeded random_seed + r, so
    replica r's start is a function of AT_SIZE_SEED + r.  FirstFit is compared with the oracle started from the replica's own values;
    FirstFitDecreasing and AllocateEntityFromQueue (the kept list, one per replica) with the mirror."""
    from test_gpu_large_launch import _launch_size, _sample

    case = cases.at_size_graph()
    R, u = _launch_size(False)
    sample = _sample(R, u, N_SAMPLE)
    kw = {} if heuristic == mirror.FIRST_FIT else dict(entity_order_keys=cases.at_size_entity_keys())
    d = _searched(case, R, cases.AT_SIZE_SEED)
    starts = _all_values(d, R)
    res = _construct(d, R, heuristic=heuristic, **kw)  # asserts out_scores == committed
    d.close()
    values = np.stack([x[0] for x in res])
    committed, fresh = np.stack([x[1] for x in res]), np.stack([x[2] for x in res])
    assert (committed == fresh).all(), np.flatnonzero((committed != fresh).any(axis=1))[:8]
    unassigned = (starts < 0).sum(axis=1)
    steps = np.asarray([x[3]["step_count"] for x in res])
    if heuristic == mirror.FIRST_FIT:
        assert (steps == unassigned).all()  # one pass: one placement per unassigned vertex
    assert (steps >= unassigned).all() and (steps <= unassigned * (unassigned + 1)).all()
    t0 = time.perf_counter()
    fired = 0
    for r in sample:
        assert (starts[r] == cases.at_size_start(oracle, case, r)).all(), r  # the start is the oracle's search seeded AT_SIZE_SEED + r
        if heuristic == mirror.FIRST_FIT:
            o = case.oracle(oracle, start=starts[r])
            base = o.stats()
            o.construct_first_fit()
            _same(res[r], o.get_vars(0, 0), o.score(), {k: o.stats()[k] - base[k] for k in ORACLE_COUNTERS}, ORACLE_COUNTERS, r)
        else:
            m = case.oracle(oracle, start=starts[r])
            st = mirror.construct(m, heuristic, n_values=case.n_values, **kw)
            _same(res[r], m.get_vars(0, 0), m.score(), st, MIRROR_COUNTERS, r)
            fired += st["kept"] >= 1 and st["step_count"] > unassigned[r]  # kept entities, retried after a later assignment
    print(f"construction at size: R={R} sample={len(sample)} heuristic={heuristic} reference+compare {time.perf_counter() - t0:.2f} s")
    assert len({tuple(starts[r]) for r in sample}) == len(sample) and (unassigned[sample] >= 10).all()
    assert heuristic == mirror.FIRST_FIT or 2 * fired >= len(sample), fired
    S = cases.AT_SIZE_SHIFT  # shift invariance: every trajectory in another wave slot, workgroup and residency
    b = _searched(case, R, cases.AT_SIZE_SEED + S)
    scores_b = b.construct_scalar(0, 0, heuristic=heuristic, **kw)
    values_b = _all_values(b, R)
    b.close()
    assert (values_b[:R - S] == values[S:]).all(), np.flatnonzero((values_b[:R - S] != values[S:]).any(axis=1))[:8]
    assert (scores_b[:R - S] == committed[S:]).all()


# ---- D. the LDS gate of the table models -------------------------------------------------------------------------------------------------
# sf_api.hip: SF_LDS_BUDGET = 160 KiB - 1 KiB; sf_api_scalar.inc: scalar_table_bytes = 12 n_values + 16 without a runs table.  Every
# host-driven kernel of the scalar class holds at most 1 KiB of static LDS (k_scalar_construct: 32 bytes, k_scalar_evaluate_moves: 32,
# k_scalar_evaluate_all: 144,
# the others none), so the budget is the edge of all of them.
LDS_BUDGET = 160 * 1024 - 1024
LAST_ADMITTED = (LDS_BUDGET - 16) // 12
LAST_BELOW_64K = (64 * 1024 - 16) // 12
GATE_MODELS = {"balance": cases.gate_balance, "assignment": cases.gate_assignment}


def test_gate_edges_are_the_ones_of_the_code():
    assert 12 * LAST_ADMITTED + 16 <= LDS_BUDGET < 12 * (LAST_ADMITTED + 1) + 16 and LAST_ADMITTED == 13566
    assert 12 * LAST_BELOW_64K + 16 <= 64 * 1024 < 12 * (LAST_BELOW_64K + 1) + 16 and LAST_BELOW_64K == 5460


@pytest.mark.parametrize("model", list(GATE_MODELS))
def test_table_model_above_the_lds_gate_is_refused_at_initialize(model):
    import solverforge_amd as sfa

    d = GATE_MODELS[model](LAST_ADMITTED + 1).gpu(1)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*per-value tables"):
        d.calculate_score()


@pytest.mark.parametrize("n_values", [LAST_BELOW_64K, LAST_BELOW_64K + 1, LAST_ADMITTED])
@pytest.mark.parametrize("model", list(GATE_MODELS))
def test_table_model_at_the_lds_gate_equals_the_oracle(oracle, model, n_values):
    import solverforge_amd as sfa

    case = GATE_MODELS[model](n_values)
    heads = cases.gate_starts(n_values)
    d, o = case.gpu(1), case.oracle(oracle)
    L = 2
    assert (d.calculate_score()[0] == o.score()[:L]).all()
    for e in (0, 1, 2, 3, 8, 11):  # apply_move: values at both ends of the tables; entities 0 and 8 share a value
        mv = (0, e, 0, 0, 0, heads[e])
        d.apply_move(mv)
        o.apply_move(mv)
        assert (d.calculate_score()[0] == o.score()[:L]).all() and (d.fresh_score()[0] == o.score()[:L]).all(), e
    top = n_values - 1
    batch = [(0, e, 0, 0, 0, v) for e in (0, 4, 5, 39) for v in (top, top - 1, 0, 63, 64, n_values // 2, heads[0])]
    batch += [(1, 0, 0, b, 0, 0) for b in (1, 2, 3, 4, 8)]  # swaps: assigned with assigned, with unassigned, of equal values
    gs, gd = d.evaluate_moves(batch)
    os_, od = o.evaluate_moves(batch)
    assert (gd == od).all() and (gs[od != 0] == os_[od != 0][:, :L]).all()
    start = o.get_vars(0, 0)
    assert (d.working_values(0, 0) == start).all()
    base = o.stats()
    o.construct_first_fit()
    _same(_construct(d, 1)[0], o.get_vars(0, 0), o.score(), {k: o.stats()[k] - base[k] for k in ORACLE_COUNTERS}, ORACLE_COUNTERS, "first fit")
    assert o.get_vars(0, 0).max() == top
    d.configure(sfa.SolverConfig(random_seed=3))
    d.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*LDS"):  # four replicas' slices per workgroup: the search gate is far lower
        d.solve_steps(12)
    d.close()
    # CheapestInsertion prices every value: 212 chunks per placement at the last admitted size (one obligation there: the mirror's time)
    for obligation in BOTH if n_values < LAST_ADMITTED else (mirror.PRESERVE_UNASSIGNED,):
        m, st = _gpu_equals_mirror(oracle, case, mirror.CHEAPEST_INSERTION, obligation, obligation=obligation)
        assert m.get_vars(0, 0).max() == top and st["moves_generated"] == case.n * n_values
