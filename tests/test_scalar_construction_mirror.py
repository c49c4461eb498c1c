"""The mirror of the scalar construction phase (tests/scalar_construction_mirror.py), pinned on the CPU:
(a) to the unchanged oracle -- mirror FirstFit / PreserveUnassigned == construct_first_fit in values, score and the two counters the oracle
    records, on every model of the GPU parity tests, with the results the oracle gives on the issue's inputs asserted as literals;
(b) to the literals of the reference's own forager / phase tests (tests/golden/scalar_construction_literals.json), through a stand-in with
    the oracle Model's four primitives whose candidate value v scores v.
The seven live-refresh heuristics and the value-candidate limit have no counterpart in the oracle: they are pinned to the mirror only
(DESIGN §19); what is checked of them here is the mirror's own consistency -- incremental == fresh score, the counters' identities, and that
the retry rule really fires.
(c) The last section asserts, on the mirror / oracle alone, that every case of tests/test_gpu_scalar_construct_wide.py has the shape it
    claims: which ordinal of a 130-candidate placement is taken, that values >= 64 are constructed, that the at-size starts are diverged."""
import json
import os

import numpy as np
import pytest

import scalar_construction_cases as cases
import scalar_construction_mirror as mirror

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_construction_literals.json")


def _mirror_kwargs(case, **kw):
    return dict(n_values=case.n_values, value_lists=case.value_lists, **kw)


# ---- (a) the oracle's construct_first_fit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(5))
def test_first_fit_equals_oracle_on_the_recorded_inputs(oracle, idx):
    case, unassigned, trials, values = cases.first_fit_inputs()[idx]
    o = case.oracle(oracle)
    o.construct_first_fit()
    got = o.get_vars(0, 0)
    assert int((got < 0).sum()) == unassigned and o.stats()["score_calculations"] == trials == o.stats()["moves_evaluated"]
    if values is not None:
        assert got.tolist() == values
    assert (o.score() == o.fresh_score()).all()
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.FIRST_FIT, **_mirror_kwargs(case))
    assert (m.get_vars(0, 0) == got).all() and (m.score() == o.score()).all()
    assert st["moves_evaluated"] == trials and st["score_calculations"] == trials and st["moves_generated"] == trials
    assert st["step_count"] == case.n and st["moves_accepted"] == case.n - unassigned == st["moves_applied"] and st["kept"] == unassigned


@pytest.mark.parametrize("idx", range(6))
def test_first_fit_equals_oracle_on_every_constraint_form(oracle, idx):
    case = cases.other_first_fit_cases()[idx]
    o = case.oracle(oracle)
    o.construct_first_fit()
    assert (o.score() == o.fresh_score()).all() and o.stats()["moves_evaluated"] > 0
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.FIRST_FIT, **_mirror_kwargs(case))
    assert (m.get_vars(0, 0) == o.get_vars(0, 0)).all() and (m.score() == o.score()).all() and (m.score() == m.fresh_score()).all()
    assert st["moves_evaluated"] == o.stats()["moves_evaluated"] and st["score_calculations"] == o.stats()["score_calculations"]


def test_first_fit_equals_oracle_with_value_lists(oracle):
    case = cases.graph(40, 150, 5, 4, value_lists=cases.ragged_lists(40, 5))
    o = case.oracle(oracle)
    o.construct_first_fit()
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.FIRST_FIT, **_mirror_kwargs(case))
    got = m.get_vars(0, 0)
    assert (got == o.get_vars(0, 0)).all() and (m.score() == o.score()).all() and got[2] == -1 and got[5] in (-1, 4)
    assert st["moves_evaluated"] == o.stats()["moves_evaluated"] and st["step_count"] == 39  # the entity without values is no placement


# ---- (b) the reference's own literals ----------------------------------------------------------------------------------------------
class ScoredToy:
    """The reference tests' ScoredDirector as the oracle Model's primitives: `entities` nullable entities, candidate ordinal k of any entity
    holds the value table[k] and the score is the sum of the held values (flat: always 0; completion: incomplete / complete)."""

    def __init__(self, table, entities=1, flat=False, completion=None, start=None):
        self.table, self.vals, self.flat, self.completion = list(table), [-1] * entities if start is None else list(start), flat, completion

    def get_vars(self, desc=0, var=0):
        return np.asarray(self.vals, dtype=np.int64)

    def _score_of(self, vals):
        if self.flat:
            return 0
        if self.completion is not None:
            return self.completion[1] if all(v >= 0 for v in vals) else self.completion[0]
        return sum(self.table[v] for v in vals if v >= 0)

    def score(self):
        return np.asarray([self._score_of(self.vals), 0, 0, 0], dtype=np.int64)

    def evaluate_moves(self, records):
        sc = np.zeros((len(records), 4), dtype=np.int64)
        do = np.zeros(len(records), dtype=np.int32)
        for i, (_, e, _, _, _, v) in enumerate(records):
            do[i] = self.vals[e] != v
            sc[i, 0] = self._score_of(self.vals[:e] + [v] + self.vals[e + 1:])
        return sc, do

    def apply_move(self, record):
        self.vals[record[1]] = record[5]


def _literals():
    return json.load(open(GOLDEN))


def test_golden_names_its_source():
    assert all(f in _literals()["source"] for f in ("forager/tests.rs", "selection.rs", "placer/tests.rs"))


@pytest.mark.parametrize("idx", range(11))
def test_forager_literals(idx):
    lit = _literals()["forager"][idx]
    toy = ScoredToy(lit["values"], flat=lit.get("flat_score", False))
    k = len(lit["values"])
    mirror.construct(toy, getattr(mirror, lit["heuristic"]), allows_unassigned=lit["keep_current_legal"], n_values=k, value_order_keys=lit["values"])
    assert (None if toy.vals[0] < 0 else toy.vals[0]) == lit["select"], lit["test"]


@pytest.mark.parametrize("idx", range(9))
def test_phase_literals(idx):
    lit = _literals()["phase"][idx]
    toy = ScoredToy(lit["values"])
    st = mirror.construct(toy, getattr(mirror, lit["heuristic"]), obligation=getattr(mirror, lit["obligation"]), allows_unassigned=lit["keep_current_legal"],
                          n_values=len(lit["values"]))
    assert (None if toy.vals[0] < 0 else lit["values"][toy.vals[0]]) == lit["value"], lit["test"]
    assert int(toy.score()[0]) == lit["score"] and st["moves_accepted"] == lit["moves_accepted"] == st["moves_applied"]
    assert st["step_count"] == lit.get("step_count", st["step_count"])


@pytest.mark.parametrize("idx", range(4))
def test_placer_literals(idx):
    """placer/tests.rs: an entity that holds a value is no placement, every other entity is one with all its candidate values, in the
    heuristic's entity order (the sorted placer's descending index = FirstFitDecreasing with key = index)."""
    lit = _literals()["placer"][idx]
    toy = ScoredToy([0, 1, 2], flat=True, start=[0 if held else -1 for held in lit["initialized"]])
    st = mirror.construct(toy, getattr(mirror, lit["heuristic"]), allows_unassigned=False, n_values=3, entity_order_keys=lit.get("entity_order_keys"))
    assert st["placements"] == lit["placements"] and st["step_count"] == len(lit["placements"]), lit["test"]
    assert all(c == lit.get("candidates_per_placement", c) for c in st["candidates"]) and st["moves_generated"] == lit.get("moves_generated", st["moves_generated"])


def test_plateau_and_nqueens_literals(oracle):
    lit = _literals()["plateau"]
    toy = ScoredToy(lit["values"], entities=lit["entities"], completion=(lit["incomplete_score"], lit["complete_score"]))
    st = mirror.construct(toy, mirror.CHEAPEST_INSERTION, n_values=1)
    assert [lit["values"][v] for v in toy.vals] == lit["result"] and int(toy.score()[0]) == lit["score"] and st["moves_accepted"] == lit["moves_accepted"]
    lit = _literals()["nqueens4_best_fit"]
    o = oracle.Model.nqueens(np.full(lit["queens"], -1, dtype=np.int64))
    st = mirror.construct(o, mirror.CHEAPEST_INSERTION, allows_unassigned=False, n_values=lit["queens"])
    assert st["moves_evaluated"] == lit["moves_evaluated"] and (o.get_vars(0, 0) >= 0).all()


# ---- the mirror's own consistency on the heuristics the oracle does not have ---------------------------------------------------------
@pytest.mark.parametrize("obligation", [mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS])
@pytest.mark.parametrize("heuristic", mirror.HEURISTICS)
def test_every_heuristic_keeps_the_score_incremental(oracle, heuristic, obligation):
    for case in (cases.graph(40, 150, 5, 4), cases.balance(), cases.assignment()):
        m = case.oracle(oracle)
        st = mirror.construct(m, heuristic, obligation=obligation, entity_order_keys=cases.keys(case.n, 4, 21), value_order_keys=cases.keys(case.n_values, 3, 22),
                              **_mirror_kwargs(case))
        assert (m.score() == m.fresh_score()).all()
        vals = m.get_vars(0, 0)
        assert st["moves_accepted"] == int((vals >= 0).sum()) and st["step_count"] == st["moves_accepted"] + st["kept"]
        assert st["moves_generated"] == st["moves_evaluated"] and st["moves_not_doable"] == 0
        if obligation == mirror.ASSIGN_WHEN_CANDIDATE_EXISTS:
            assert (vals >= 0).all() and st["kept"] == 0
            if heuristic not in (mirror.CHEAPEST_INSERTION,):  # unscored picks: first doable / extreme strength
                assert st["score_calculations"] == 0


@pytest.mark.parametrize("heuristic", mirror.LIVE_REFRESH)
def test_live_refresh_retries_the_kept_entities(oracle, heuristic):
    """cases.retry_assignment: entities keep current until a rewarded entity has opened a value row; that assignment advances the solution
    revision, the kept entities are placed again from the head of the order, and the open row takes them.  One pass leaves them unassigned."""
    case = cases.retry_assignment()
    m = case.oracle(oracle)
    st = mirror.construct(m, heuristic, entity_order_keys=cases.RETRY_ENTITY_KEYS, value_order_keys=cases.retry_value_keys(heuristic), **_mirror_kwargs(case))
    assert st["kept"] >= 1 and st["assigned_on_retry"] >= 1 and st["step_count"] > case.n and (m.get_vars(0, 0) >= 0).all()
    assert (m.score() == m.fresh_score()).all()
    one_pass = case.oracle(oracle)
    st1 = mirror.construct(one_pass, mirror.FIRST_FIT, **_mirror_kwargs(case))
    assert st1["assigned_on_retry"] == 0 and st1["step_count"] == case.n and (one_pass.get_vars(0, 0) < 0).sum() == 7


def test_long_retry_case_leaves_the_kept_list_from_its_middle(oracle):
    """What the GPU test of the multi-chunk kept list rests on: more than 64 entities are kept when the opener assigns, the entities without
    value 1 stay kept, so the assignments on retry come from the middle of the list."""
    case = cases.long_retry_assignment()
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.ALLOCATE_ENTITY_FROM_QUEUE, entity_order_keys=np.zeros(case.n, dtype=np.int64), **_mirror_kwargs(case))
    vals = m.get_vars(0, 0)
    assert st["placements"][:121] == list(range(121)) and st["assigned_on_retry"] == 80 and (vals[1::3] < 0).all() and (vals[0::3] == 1).all()
    first_retry = st["placements"][121:124]
    assert first_retry == [0, 1, 2]  # 0 is assigned (head of the list), the restart keeps 1 and assigns 2 from the middle
    assert (m.score() == m.fresh_score()).all()


def test_timetable_primitives_are_consistent():
    case = cases.timetable()
    m = case.oracle(None)
    st = mirror.construct(m, mirror.CHEAPEST_INSERTION, **_mirror_kwargs(case))
    assert st["moves_evaluated"] == 64 * 8 and m.score()[0] < 0 and m.score()[1] < 0  # both levels carry matches: the choice reads both


def test_value_candidate_limit_cuts_before_the_value_order(oracle):
    case = cases.assignment()
    m = case.oracle(oracle)
    mirror.construct(m, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, obligation=mirror.ASSIGN_WHEN_CANDIDATE_EXISTS, value_candidate_limit=3,
                     value_order_keys=[5, 4, 3, 2, 1, 0, 0], **_mirror_kwargs(case))
    assert (m.get_vars(0, 0) == 2).all()  # the first three values in descending-key order: value 2 leads, and the forced first fit takes it


# ---- the product without a device ---------------------------------------------------------------------------------------------------
def test_construct_scalar_fails_loudly_without_device():
    import ctypes as C

    from solverforge_amd import _lib

    L = _lib.load()
    cfg = _lib.ScalarConstructionConfigStruct(0, 0, 0, 0)
    rc = L.sf_construct_scalar(None, 0, 0, C.byref(cfg), None, None, None)
    if L.sf_device_count() > 0:
        assert _lib.ERRORS[rc] == "SF_ERR_INVALID"  # a device exists: the NULL context is the error
    else:
        assert _lib.ERRORS[rc] == "SF_ERR_NO_DEVICE"


# ---- the shapes the wide GPU cases rest on (tests/test_gpu_scalar_construct_wide.py), on the mirror / oracle alone ------------------------
BOTH = (mirror.PRESERVE_UNASSIGNED, mirror.ASSIGN_WHEN_CANDIDATE_EXISTS)
STRENGTH = (mirror.WEAKEST_FIT, mirror.WEAKEST_FIT_DECREASING, mirror.STRONGEST_FIT, mirror.STRONGEST_FIT_DECREASING)
LIMITS = (63, 64, 65, 129, 131)


def _ordinals(case, vals):
    """The ordinal of each assigned entity's value in its candidate list."""
    return {e: (case.value_lists[e].index(int(v)) if case.value_lists is not None else int(v)) for e, v in enumerate(vals) if v >= 0}


def test_wide_best_fit_takes_the_named_ordinals(oracle):
    case = cases.best_fit_assignment(ex_level=-1)
    for obligation in BOTH:
        m = case.oracle(oracle)
        st = mirror.construct(m, mirror.CHEAPEST_INSERTION, obligation=obligation, **_mirror_kwargs(case))
        assert m.get_vars(0, 0)[:10].tolist() == [0, 63, 64, 65, 127, 128, 129, 10, 70, 0] == cases.BEST_FIT_VALUES
        assert st["moves_generated"] == 3120 == st["score_calculations"] and st["step_count"] == 24 == st["moves_accepted"]


def test_wide_best_fit_keeps_current_after_the_last_chunk(oracle):
    """The exists node on the hard level: a row costs what the unassigned penalty gives back and every cost is positive, so the baseline is
    strictly greater than the best of the 130 trials -- of the last chunk's too."""
    case = cases.best_fit_assignment(ex_level=0)
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.CHEAPEST_INSERTION, **_mirror_kwargs(case))
    assert st["kept"] >= 1 and st["candidates"][0] == 130 and st["placements"][0] == 0 and m.get_vars(0, 0)[0] == -1
    assert st["score_calculations"] == 130 * st["step_count"]
    forced = case.oracle(oracle)
    st = mirror.construct(forced, mirror.CHEAPEST_INSERTION, obligation=mirror.ASSIGN_WHEN_CANDIDATE_EXISTS, **_mirror_kwargs(case))
    assert forced.get_vars(0, 0)[0] == 0 and st["kept"] == 0  # entity 0 opens its best row


@pytest.mark.parametrize("heuristic", STRENGTH)
def test_wide_strength_extremes_sit_where_the_case_says(oracle, heuristic):
    case = cases.wide_assignment()
    ek = cases.keys(case.n, 4, 21)
    for name, (vk, limit, want) in cases.strength_keys(heuristic in (mirror.WEAKEST_FIT, mirror.WEAKEST_FIT_DECREASING)).items():
        for obligation in BOTH:
            m = case.oracle(oracle)
            st = mirror.construct(m, heuristic, obligation=obligation, value_candidate_limit=limit, entity_order_keys=ek, value_order_keys=vk, **_mirror_kwargs(case))
            assert (m.get_vars(0, 0) == want).all(), (name, obligation)
            assert st["moves_generated"] == case.n * (limit or 130)


@pytest.mark.parametrize("heuristic", STRENGTH)
def test_wide_lists_put_the_extreme_in_every_chunk(oracle, heuristic):
    case = cases.wide_assignment(value_lists=cases.wide_lists(24))
    assert sorted({len(l) for l in case.value_lists}) == cases.WIDE_LENGTHS and all(len(set(l)) == len(l) for l in case.value_lists)
    m = case.oracle(oracle)
    mirror.construct(m, heuristic, entity_order_keys=cases.keys(case.n, 4, 21), value_order_keys=cases.wide_list_keys(), **_mirror_kwargs(case))
    vals = m.get_vars(0, 0)
    assert (vals >= 0).all()
    got = _ordinals(case, vals)
    which = 2 if heuristic in (mirror.WEAKEST_FIT, mirror.WEAKEST_FIT_DECREASING) else 1
    for e, placed in cases.WIDE_PLACED.items():
        assert got[e] == placed[which], (e, got[e])
    chosen = set(got.values())
    assert any(k < 64 for k in chosen) and any(64 <= k < 128 for k in chosen) and any(k >= 128 for k in chosen)
    assert chosen & {64, 128} and chosen & {127}  # lane 0 and lane 63 of a later chunk
    assert len(chosen) >= 12  # the entities' extremes sit at different ordinals


def test_wide_value_queue_never_passes_the_cut(oracle):
    vk = cases.keys(cases.WIDE, 7, 71)
    lists = cases.wide_lists(100)
    for case in (cases.wide_clique(100), cases.wide_clique(100, value_lists=lists)):
        deepest = 0
        for limit in (0,) + LIMITS:
            m = case.oracle(oracle)
            st = mirror.construct(m, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE, value_candidate_limit=limit, value_order_keys=vk, **_mirror_kwargs(case))
            got = _ordinals(case, m.get_vars(0, 0))
            assert all(k < (limit or 131) for k in got.values()), limit  # the cut comes before the sort
            assert (m.score() == m.fresh_score()).all() and m.score()[0] == -st_unassigned(m)
            if case.value_lists is None:
                assert len(got) == min(limit or 130, 100)  # a clique: one colour each, and nothing beyond the cut
            deepest = max(deepest, len(got))
        assert deepest > 64  # the sorted order was walked past its first chunk: every taken colour lies before the one an entity takes


def st_unassigned(m):
    return int((m.get_vars(0, 0) < 0).sum())


@pytest.mark.parametrize("n,k,hits", [(70, 80, cases.ROTATED_HITS_70), (130, 140, cases.ROTATED_HITS_130)])
def test_rotated_lists_hit_at_the_named_ordinals(oracle, n, k, hits):
    case = cases.rotated_clique(n, k, hits)
    o = case.oracle(oracle)
    o.construct_first_fit()
    assert o.get_vars(0, 0).tolist() == list(range(n))  # entity e takes colour e ...
    got = _ordinals(case, o.get_vars(0, 0))
    assert all(got[e] == at for e, at in hits.items()) and {63, 64} <= set(hits.values())  # ... at the ordinal its rotation fixes
    assert o.stats()["score_calculations"] == sum(k + 1 for k in got.values())
    m = case.oracle(oracle)
    st = mirror.construct(m, mirror.FIRST_FIT, **_mirror_kwargs(case))
    assert (m.get_vars(0, 0) == o.get_vars(0, 0)).all() and st["score_calculations"] == o.stats()["score_calculations"]


@pytest.mark.parametrize("heuristic", mirror.LIVE_REFRESH)
def test_wide_live_refresh_retries_through_a_row_of_a_later_chunk(oracle, heuristic):
    case = cases.wide_retry_assignment()
    m = case.oracle(oracle)
    st = mirror.construct(m, heuristic, entity_order_keys=cases.RETRY_ENTITY_KEYS, value_order_keys=cases.wide_retry_value_keys(heuristic), **_mirror_kwargs(case))
    assert st["kept"] >= 1 and st["assigned_on_retry"] >= 1 and st["step_count"] > case.n
    vals = m.get_vars(0, 0)
    assert min(cases.WIDE_RETRY_ROWS) >= 64 and (vals[vals >= 0] >= 64).all() and (vals == cases.WIDE_RETRY_ROWS[0]).sum() > 1


@pytest.mark.parametrize("name", list(cases.wide_table_models()))
def test_wide_table_models_use_values_past_the_first_chunk(oracle, name):
    """Every heuristic of the GPU test assigns values >= 64 on every model: scalar_tables_apply and the statistics of the balance models are
    driven at table indices beyond the first round of lanes."""
    make = cases.wide_table_models()[name]
    case = make(None)
    assert case.n > 64 and case.n_values >= 65 and (12 * case.n_values) % 16 != 0
    ek = cases.keys(case.n, 4, 21)
    for heuristic in (mirror.CHEAPEST_INSERTION, mirror.STRONGEST_FIT_DECREASING, mirror.ALLOCATE_TO_VALUE_FROM_QUEUE):
        vk = cases.table_keys(case.n_values, least=heuristic == mirror.ALLOCATE_TO_VALUE_FROM_QUEUE)
        for obligation in BOTH:
            m = case.oracle(oracle)
            mirror.construct(m, heuristic, obligation=obligation, entity_order_keys=ek, value_order_keys=vk, **_mirror_kwargs(case))
            assert (m.score() == m.fresh_score()).all(), (heuristic, obligation)
            # (fairness over the bins in use, cap -2: one bin is perfectly fair, so the best fit never opens a second one)
            assert m.get_vars(0, 0).max() >= 64 or (heuristic == mirror.CHEAPEST_INSERTION and name.startswith("balance-2")), (heuristic, obligation)
    listed = make(cases.rotated_lists(case.n, case.n_values))  # first fit takes the head of the list: the lists spread the heads over the range
    o = listed.oracle(oracle)
    o.construct_first_fit()
    assert o.get_vars(0, 0).max() >= 64 and (o.score() == o.fresh_score()).all()
    for obligation in BOTH:
        m = listed.oracle(oracle)
        mirror.construct(m, mirror.FIRST_FIT, obligation=obligation, **_mirror_kwargs(listed))
        assert m.get_vars(0, 0).max() >= 64
        if obligation == mirror.PRESERVE_UNASSIGNED:
            assert (m.get_vars(0, 0) == o.get_vars(0, 0)).all()


def test_at_size_starts_are_diverged_and_leave_work_to_the_kept_list(oracle):
    """What the at-size GPU test rests on: the graph has the edges it claims, FirstFit leaves vertices unassigned, the searched starts of
    different seeds differ and leave at least 10 vertices unassigned each, and at least half of the live-refresh runs keep entities and retry them."""
    case = cases.at_size_graph()
    o = case.oracle(oracle)
    o.construct_first_fit()
    assert (o.get_vars(0, 0) < 0).sum() >= 5
    from solverforge_amd import datasets

    g = datasets.make_graph(40, 180, 3, seed=13)
    assert len(g["adj"]) == 2 * 180 and g["n_colors"] == 3
    sample = [0, 1, 3, 4, 5, 63, 64, 16383, 16384, 16420, 8191, 8192]
    starts = [cases.at_size_start(oracle, case, r) for r in sample]
    assert len({tuple(s) for s in starts}) == len(starts) and all((s < 0).sum() >= 10 for s in starts) and all((s >= 0).any() for s in starts)
    for heuristic in (mirror.FIRST_FIT_DECREASING, mirror.ALLOCATE_ENTITY_FROM_QUEUE):
        fired = 0
        for s in starts:
            m = case.oracle(oracle, start=s)
            st = mirror.construct(m, heuristic, entity_order_keys=cases.at_size_entity_keys(), **_mirror_kwargs(case))
            assert (m.score() == m.fresh_score()).all()
            # In graph colouring a kept vertex is never assigned later: every colour of it conflicts, and a construction only adds
            # neighbours' colours.  What the kept list does here is to be retried, whole, after every later assignment.
            assert st["assigned_on_retry"] == 0
            fired += st["kept"] >= 1 and st["step_count"] > int((s < 0).sum())
        assert 2 * fired >= len(starts), (heuristic, fired)
