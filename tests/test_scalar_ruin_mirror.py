"""CPU: the mirror of the scalar ruin-and-recreate leaf (tests/scalar_ruin_mirror.py) against the reference's own literals
(tests/golden/scalar_ruin_goldens.json), its random_range against the oracle's, and -- on the mirror alone -- that the model scripts of
tests/scalar_ruin_cases.py reach every edge of the rule the GPU tests rely on."""
import numpy as np
import pytest

import scalar_ruin_cases as rc
import scalar_ruin_mirror as rm

_runs = {}


class Plan:
    """The test double of descriptor/tests/mod/ruin_recreate.rs: tasks choose a worker, the score is a function of the worker."""

    def __init__(self, tasks, unassigned_score, assigned_scores):
        self.tasks, self.un, self.sc = [(-1 if t is None else t) for t in tasks], unassigned_score, list(assigned_scores)

    def score(self):
        return np.array([sum(self.un if t < 0 else self.sc[t] for t in self.tasks), 0, 0, 0], dtype=np.int64)

    def get_vars(self, desc, var):
        return np.array(self.tasks, dtype=np.int64)

    def apply_move(self, move):
        self.tasks[move[1]] = move[5]

    def evaluate_moves(self, moves):
        scores, doable = np.zeros((len(moves), 4), dtype=np.int64), np.zeros(len(moves), dtype=np.int32)
        for i, mv in enumerate(moves):
            old = self.tasks[mv[1]]
            if old == mv[5] or not 0 <= mv[5] < len(self.sc):
                continue
            self.tasks[mv[1]] = mv[5]
            scores[i], doable[i] = self.score(), 1
            self.tasks[mv[1]] = old
        return scores, doable


def _leaf(oracle, case, plan, seed=0):
    recreate = rm.FIRST_FIT if case["recreate"] == "first_fit" else rm.CHEAPEST_INSERTION
    return rm.RuinLeaf(oracle, plan, len(plan.tasks), case["workers"], seed, min_ruin_count=case.get("min_ruin_count", 1), max_ruin_count=case.get("max_ruin_count", 1),
                       moves_per_step=case.get("moves_per_step", 1), value_candidate_limit=case["value_candidate_limit"], recreate=recreate,
                       allows_unassigned=case["allows_unassigned"], levels=1)


def test_reference_literals(oracle):
    g = rm.golden_file()
    ctx = rm.Context(oracle, 0, 0, rm.ORDER_ORIGINAL)
    for case in g["moves"]:
        plan = Plan(case["tasks"], case["unassigned_score"], case["assigned_scores"])
        leaf = _leaf(oracle, case, plan)
        emitted = [row for row in leaf.open(ctx) if row["emitted"]]
        assert len(emitted) == case["expect_moves"], case["name"]
        assert plan.tasks == case["tasks"], case["name"]  # a cursor open leaves the solution as it was
        if emitted:
            leaf.commit(emitted[0])
        assert plan.tasks == case["expect_tasks"], case["name"]
    for case in g["direct_moves"]:
        plan = Plan(case["tasks"], 0, [0] * case["workers"])
        leaf = _leaf(oracle, case, plan)
        assert leaf.is_doable(case["entities"]) == case["expect_doable"], case["name"]
        assert plan.tasks == case["expect_tasks"], case["name"]  # do_move of a move that is not doable changes nothing (apply.rs:162-164)
    s = g["seeds"]
    batches = {}
    for key in ("first", "repeat", "changed"):
        plan = Plan(s["tasks"], 0, [0] * s["workers"])
        batches[key] = [row["entities"] for row in _leaf(oracle, s, plan, seed=s[key]).open(ctx) if row["emitted"]]
    assert batches["first"] == batches["repeat"] and batches["first"] != batches["changed"] and len(batches["first"]) == s["moves_per_step"]
    for mn, mx in g["bounds"]["rejected"]:
        assert rm.check_bounds(mn, mx) is not None
    for mn, mx in g["bounds"]["accepted"]:
        assert rm.check_bounds(mn, mx) is None


@pytest.mark.parametrize("low,high", [(0, 0), (5, 5), (0, 1), (3, 4), (0, 2), (2, 7), (0, 39), (1, 65536), (0, 99999), (0, (1 << 32) - 2)])
def test_random_range_is_the_oracles(oracle, low, high):
    for seed in (0, 17, 0xDEADBEEFCAFEF00D):
        want = oracle.random_range_stream(seed, low, high, 200)
        s = rm.Stream(oracle, seed)
        assert [s.random_range(low, high) for _ in range(200)] == [int(x) for x in want]


def test_selection_index_is_the_oracles(oracle):
    for order in (0, 3, 4):
        ctx = rm.Context(oracle, 7, 0x1234567, order)
        for n in (1, 2, 10, 16):
            got = [ctx.selection_index(k, n, rm.SALT_ORDER) for k in range(n)]
            assert got == [oracle.lib().sfo_ctx_selection_index(7, 0x1234567, order, k, n, rm.SALT_ORDER) for k in range(n)]


def _run(oracle, name):
    """The script on the mirror: its step records (shared by the tests below; the models are rebuilt per script, the records are not changed)."""
    if name not in _runs:
        o, search = rc.search_of(oracle, name)
        recs = []
        for _ in range(rc.SCRIPTS[name]["steps"]):
            before, current = search.leaf.values(), search.current
            rec = search.step()
            rec["before"], rec["current"] = before, current
            recs.append(rec)
        _runs[name] = (recs, search)
    return _runs[name]


def _rows(oracle, name):
    return [(rec, row) for rec in _run(oracle, name)[0] for row in rec["table"]]


@pytest.mark.parametrize("name", list(rc.SCRIPTS))
def test_every_script_runs_and_moves(oracle, name):
    recs, search = _run(oracle, name)
    assert search.stats["step_count"] == rc.SCRIPTS[name]["steps"]
    assert search.leaf.score() == search.current
    if name != "required_limit_zero":
        assert any(row["emitted"] for rec in recs for row in rec["table"])


def test_edge_1_batch_without_an_assigned_entity(oracle):
    assert any(not row["emitted"] and row["entities"] and all(rec["before"][e] < 0 for e in row["entities"]) for rec, row in _rows(oracle, "colouring_sparse_start"))
    assert any(row["emitted"] for _, row in _rows(oracle, "colouring_sparse_start"))


def test_edge_2_required_entity_with_an_empty_value_list(oracle):
    lists = rc.problem("required_empty_list")["value_lists"]
    rows = _rows(oracle, "required_empty_list")
    assert any(not row["emitted"] and any(not lists[e] for e in row["entities"]) for _, row in rows)
    assert any(row["emitted"] for _, row in rows)
    assert all(v >= 0 for _, row in rows if row["emitted"] for v in row["values"])  # a required variable: first fit without a baseline always places


def test_edge_3_limit_zero_emits_nothing_and_the_stream_advances(oracle):
    recs, search = _run(oracle, "required_limit_zero")
    assert len(recs) == 3 and all(not row["emitted"] for rec in recs for row in rec["table"]) and all(rec["consumed"] == 0 for rec in recs)
    tables = [[row["entities"] for row in rec["table"]] for rec in recs]
    assert tables[0] != tables[1] != tables[2] and search.leaf.rng.pos > 0
    assert search.stats == {k: (3 if k == "step_count" else 0) for k in rm.COUNTERS}


def test_edge_4_clamping_and_the_count_draw(oracle):
    rows = _rows(oracle, "three_entities")
    assert all(2 <= len(row["entities"]) <= 3 for _, row in rows) and {len(row["entities"]) for _, row in rows} == {2, 3}
    assert all(len(row["entities"]) == 3 for _, row in _rows(oracle, "colouring_original"))  # min == max: no count draw
    s0, s1 = rm.Stream(oracle, 1), rm.Stream(oracle, 1)
    rm.generate_ruin_batches(40, 3, 3, 6, s0)  # six batches of three swaps; a draw takes one word of the stream, rarely two
    b1 = rm.generate_ruin_batches(40, 2, 3, 6, s1)  # ... and one more draw per batch for the count
    assert 18 <= s0.pos <= 21 and s1.pos >= 6 + sum(len(b) for b in b1)


def test_edge_5_random_repeats_a_batch_and_shuffled_does_not(oracle):
    assert any(len({tuple(row["entities"]) for row in rec["table"]}) < len(rec["table"]) for rec in _run(oracle, "colouring_ff")[0])
    for step in range(6):  # Shuffled: a start plus a stride, every drawn batch once
        ctx = rm.Context(oracle, step, oracle.lib().sfo_step_seed(6, step), rm.ORDER_SHUFFLED)
        assert sorted(ctx.apply_selection_order(list(range(10)), rm.SALT_ORDER)) == list(range(10))
    assert any(ctx.apply_selection_order(list(range(10)), rm.SALT_ORDER) != list(range(10)) for ctx in [rm.Context(oracle, 1, 99, rm.ORDER_SHUFFLED)])


def test_edge_6_first_fit_with_and_without_a_baseline(oracle):
    assert any(row["emitted"] and -1 in row["values"] for _, row in _rows(oracle, "colouring_ff"))  # nothing strictly above the baseline: left unassigned
    lists = rc.problem("required_empty_list")["value_lists"]
    rows = [row for _, row in _rows(oracle, "required_empty_list") if row["emitted"]]
    assert rows and all(v == lists[e][0] for row in rows for e, v in zip(row["entities"], row["values"]))  # no baseline: ordinal 0


def test_edge_7_cheapest_insertion_ordinals_ties_and_the_baseline(oracle):
    placed = {}
    for _, row in _rows(oracle, "assignment_range"):
        if row["emitted"]:
            for e, v in zip(row["entities"], row["values"]):
                placed.setdefault(e % 5 if e != 5 else "twice", set()).add(v)
    for k, ordinal in enumerate(rc.BEST_ORDINALS):
        assert placed.get(k) == {ordinal}, (k, placed.get(k))
    assert placed.get("twice") == {10}  # the best twice: the first wins
    # a recreate that ends exactly at the baseline is taken (>=): a vertex whose best colour costs one conflict, what staying unassigned costs
    hit = False
    for name in ("colouring_ci", "wide_16x8"):
        p = rc.problem(name)
        for rec, row in _rows(oracle, name):
            if not row["emitted"]:
                continue
            vals = list(rec["before"])
            for e in row["entities"]:
                vals[e] = -1
            for e, v in zip(row["entities"], row["values"]):
                nb = p["adj"][p["adj_off"][e]:p["adj_off"][e + 1]]
                conflicts = [sum(1 for u in nb if vals[u] == c) for c in range(p["n_colors"])]
                if v >= 0:
                    assert conflicts[v] == min(conflicts) and conflicts[v] <= 1 and v == conflicts.index(min(conflicts))
                    hit = hit or conflicts[v] == 1
                else:
                    assert min(conflicts) >= 2
                vals[e] = v
    assert hit


def test_edge_8_the_second_placement_depends_on_the_first(oracle):
    """A batch with two adjacent vertices: the later one's colour differs from what it would take had the earlier one not been placed."""
    found = False
    for name in ("colouring_ci", "wide_16x8", "colouring_original"):
        p = rc.problem(name)
        for rec, row in _rows(oracle, name):
            if found or not row["emitted"]:
                continue
            ents = row["entities"]
            for j in range(1, len(ents)):
                nb = set(int(u) for u in p["adj"][p["adj_off"][ents[j]]:p["adj_off"][ents[j] + 1]])
                if not any(ents[i] in nb and row["values"][i] >= 0 for i in range(j)):
                    continue
                vals = list(rec["before"])
                for e in ents:
                    vals[e] = -1
                o = rc.oracle_model(oracle, name, np.array(vals, dtype=np.int64))
                alone = rc.leaf_of(oracle, name, o).do_move([ents[j]])[1][0]
                found = found or alone != row["values"][j]
    assert found


def test_edge_9_a_recreate_that_restores_the_old_values(oracle):
    hit = [(rec, row) for name in ("colouring_ci", "assignment_range", "balance_fair") for rec, row in _rows(oracle, name)
           if row["emitted"] and row["values"] == [rec["before"][e] for e in row["entities"]]]
    assert hit
    for rec, row in hit:
        assert row["score"] == rec["current"]
    # its score is the step's current score: such a candidate is never accepted by HillClimbing
    recs = _run(oracle, "assignment_range")[0]
    for rec in recs:
        for c, ok in zip(rec["candidates"], rec["accepted"]):
            if c["row"] is not None and c["row"]["values"] == [rec["before"][e] for e in c["row"]["entities"]]:
                assert not ok


def test_edge_10_the_limit_cuts_a_value_list(oracle):
    lists = rc.problem("assignment_lists")["value_lists"]
    limit = rc.SCRIPTS["assignment_lists"]["leaf"]["value_candidate_limit"]
    assert all(len(l) > limit for l in lists)
    placed = [(e, v) for _, row in _rows(oracle, "assignment_lists") if row["emitted"] for e, v in zip(row["entities"], row["values"])]
    assert any(rc.BEST_ORDINALS[e % 5] >= limit and e != 5 for e, v in placed)  # the cheapest value lies beyond the cut ...
    assert all(0 <= v < limit for e, v in placed)  # ... and is not taken


def test_counters_of_one_step(oracle):
    """One generated, evaluated and scored candidate per pull, none not doable; the inner trials are no candidates."""
    recs, search = _run(oracle, "colouring_ff")
    st = search.stats
    assert st["moves_generated"] == st["moves_evaluated"] == st["score_calculations"] == sum(r["consumed"] for r in recs) and st["moves_not_doable"] == 0
    assert st["moves_applied"] == sum(1 for r in recs if r["pick"] is not None) and search.leaf.inner_trials > st["moves_generated"]
