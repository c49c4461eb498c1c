"""The mirror of the scalar construction phase (tests/scalar_construction_mirror.py), pinned on the CPU:
(a) to the unchanged oracle -- mirror FirstFit / PreserveUnassigned == construct_first_fit in values, score and the two counters the oracle
    records, on every model of the GPU parity tests, with the results the oracle gives on the issue's inputs asserted as literals;
(b) to the literals of the reference's own forager / phase tests (tests/golden/scalar_construction_literals.json), through a stand-in with
    the oracle Model's four primitives whose candidate value v scores v.
The seven live-refresh heuristics and the value-candidate limit have no counterpart in the oracle: they are pinned to the mirror only
(DESIGN §19); what is checked of them here is the mirror's own consistency -- incremental == fresh score, the counters' identities, and that
the retry rule really fires."""
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
