"""CPU: tests/vnd_mirror.py (the Variable Neighborhood Descent phase restated, vnd/phase.rs:31-167,181-404) over the reference's own unit
test (tests/golden/vnd_goldens.json, as data) and over the model scripts of tests/vnd_cases.py, which together must reach every edge of
the rule -- judged on the mirror alone.  The GPU tests compare the device with this mirror, so it is pinned here without a device.  The
conditions below are conditions on the inputs, not tolerances: if a script misses one after a change to the mirror, the mirror is wrong."""
import pytest

import vnd_cases as vc
import vnd_mirror as vm

SEED = 7
_memo = {}


def _run(sfo, name):
    if name not in _memo:
        o = vc.oracle_model(sfo, name)
        ph = vm.VndPhase(o, vc.leaf_bits(name), lambda s: sfo.lib().sfo_step_seed(SEED, s))
        recs = ph.run(500)
        _memo[name] = (recs, ph, vm.is_local_optimum(o, vc.leaf_bits(name)))
    return _memo[name]


def test_the_reference_s_own_test_through_the_pick_rule():
    scripts = vm.golden_file()["scripts"]
    assert [s["name"] for s in scripts] == ["vnd_single_neighborhood_applies_best_improving_move"]
    for s in scripts:
        assert s["source"].startswith("crates/solverforge-solver/src/phase/localsearch/vnd/tests.rs:")
        hoods = [[(m["doable"], m["score"]) for m in hood] for hood in s["neighborhoods"]]
        final, picks = vm.run_scores(hoods, s["initial"])
        assert picks[0] == s["expected_first_pick"] and final == s["expected_final_score"]
        assert picks[-1] is None and len(picks) == 2  # the second step finds nothing: k == n ends the phase


def test_pick_rule_edges():
    cur = (0, 0)
    assert vm.pick([], [], cur) is None
    assert vm.pick([(0, 0), (0, -1)], [True, True], cur) is None  # equal to the current score is not an improvement
    assert vm.pick([(0, 5), (0, 9)], [True, False], cur) == 0  # a candidate that is not doable is released
    assert vm.pick([(0, 3), (0, 7), (0, 7), (0, 2)], [True] * 4, cur) == 1  # of equal bests the first pulled stays
    assert vm.pick([(-1, 100), (0, 1)], [True, True], cur) == 1  # lexicographic


# What the issue measured on the CPU oracle: steps, finds at k = 0, 1, ..., steps with tied bests, most not-doable pulls of a cursor, longest cursor
EXPECTED = {
    "cvrp_reverse_first": (35, {0: 17, 1: 7}, 16, 0, 3560),
    "cvrp_swap_first": (27, {0: 15, 1: 1, 2: 2}, None, 0, None),
    "cvrp_nearby": (36, None, None, 0, None),
    "colouring": (27, None, 22, 67, None),
    "jobshop": (15, None, None, 12, None),
}


@pytest.mark.parametrize("name", list(vc.SCRIPTS))
def test_script_on_the_mirror(oracle, name):
    recs, ph, optimum = _run(oracle, name)
    steps, finds, tied, not_doable, cursor = EXPECTED[name]
    got = {}
    for r in recs:
        if r["pick"] is not None:
            got[r["k"]] = got.get(r["k"], 0) + 1
    assert len(recs) == steps
    assert finds is None or got == finds
    assert tied is None or sum(r["ties"] >= 2 for r in recs) == tied
    assert max(r["not_doable"] for r in recs) == not_doable
    assert cursor is None or max(r["cursor"] for r in recs) == cursor
    # every script ends at k == n, in a local optimum of all its neighbourhoods
    assert ph.done and ph.k == ph.n and optimum
    found = sum(r["pick"] is not None for r in recs)
    assert ph.stats["moves_accepted"] == ph.stats["moves_applied"] == found  # the applied pick only (phase.rs:117-127)
    assert ph.stats["step_count"] == steps and ph.idle_steps == steps - found
    assert ph.stats["moves_generated"] == ph.stats["moves_evaluated"] == sum(r["cursor"] for r in recs)
    assert ph.stats["moves_not_doable"] == sum(r["not_doable"] for r in recs) == ph.stats["moves_generated"] - ph.stats["score_calculations"]
    assert [r["step_index"] for r in recs] == list(range(steps))  # a step that applies nothing is still a step
    if name == "colouring":  # the swap leaf finds once, after the change leaf ran dry
        assert got[1] == 1
    if name == "jobshop":  # every find comes from the scalar class, after both list neighbourhoods came up empty
        assert set(got) == {2}


def test_the_scripts_reach_every_edge_of_the_rule(oracle):
    recs = {name: _run(oracle, name)[0] for name in vc.SCRIPTS}
    everything = [r for rs in recs.values() for r in rs]
    assert any(r["pick"] is not None and r["k"] >= 2 for r in everything)  # a find at k >= 2
    assert any(a["pick"] is not None and a["k"] >= 1 and b["k"] == 0 for rs in recs.values() for a, b in zip(rs, rs[1:]))  # a reset from k >= 1 to 0
    assert any(r["ties"] >= 2 and r["last_tie"] != r["pick"] for r in everything)  # equal strictly-best candidates, the first is not the last
    assert any(r["cursor"] > 64 for r in everything)  # a cursor of more than one chunk
    assert any(r["pick"] is None and r["not_doable"] > 0 for r in everything)  # nothing found on a cursor that holds not-doable candidates
    assert all(_run(oracle, name)[1].done for name in vc.SCRIPTS)  # termination at k == n
