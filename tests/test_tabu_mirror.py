"""CPU: tests/tabu_mirror.py (the TabuSearch acceptor and the four fixed-size move signatures restated) over the reference's own unit tests
(tests/golden/tabu_goldens.json: call sequences and expected results as data) and over the hand-written edge scripts, each of which must
reach the edge it is named for; the stamp-table formulation of a tabu memory against the FIFO; the device packing's injectivity.  The GPU
tests compare the device with this mirror, so it is pinned here without a device."""
import itertools
import random

import pytest

import tabu_mirror as tm


def test_goldens_are_the_nine_reference_tests():
    f = tm.golden_file()
    assert len(f["scripts"]) == 9 and len({s["name"] for s in f["scripts"]}) == 9
    for s in f["scripts"]:
        assert s["name"].startswith("tabu_search_") and s["source"].startswith("crates/solverforge-solver/src/phase/localsearch/acceptor/tests.rs:")
    assert len(tm.goldens()) == 8 and all(s["ops"][0][0] == "phase_started" for s in tm.goldens())
    assert [d["kind"] for d in f["direction_stability"]] == ["scalar_swap", "list_swap"]


@pytest.mark.parametrize("script", tm.goldens(), ids=lambda s: s["name"])
def test_mirror_passes_the_reference_tests(script):
    results = tm.run(script)  # asserts every expected decision of the script
    assert sum(op[0] == "is_accepted" for op, _, _, _ in results) >= 1
    if script.get("requires_move_signatures"):
        assert [res for op, res, _, _ in results if op[0] == "is_accepted"] == ["panics"]


def test_zero_tenures_are_refused_with_the_reference_s_message():
    cases = tm.policy_error_golden()["policy_errors"]
    assert len(cases) == 4
    for case in cases:
        with pytest.raises(ValueError) as e:
            tm.TabuSearch(case["policy"])
        assert str(e.value) == case["message"]
    assert tm.normalize_policy([None, None, None, None, False]) == (None, None, 10, None, False)
    assert tm.normalize_policy({"move_only": 10}) == (None, None, 10, None, True)


def test_direction_stability_goldens():
    swap, lswap = tm.golden_file()["direction_stability"]
    scope, vals = tuple(swap["scope"]), list(swap["values"])
    fwd = tm.swap_signature(scope, *swap["forward"], vals[swap["forward"][0]], vals[swap["forward"][1]])
    l, r = swap["forward"]
    vals[l], vals[r] = vals[r], vals[l]
    rev = {k: tm.swap_signature(scope, *swap[k], vals[swap[k][0]], vals[swap[k][1]]) for k in ("reverse_same_coordinates", "reverse_flipped_coordinates")}
    assert fwd.move_id == fwd.undo_move_id == rev["reverse_same_coordinates"].move_id == rev["reverse_flipped_coordinates"].move_id
    acc = swap["acceptor"]
    a = tm.TabuSearch(acc["policy"])
    a.phase_started(acc["initial"])
    a.step_ended(acc["step_score"], fwd)
    assert a.is_accepted(acc["last_step_score"], acc["move_score"], rev[acc["candidate"]]) is acc["accepted"]
    scope, lists = tuple(lswap["scope"]), [list(x) for x in lswap["lists"]]
    sig = lambda c: tm.list_swap_signature(scope, c[0], c[1], lists[c[0]][c[1]], c[2], c[3], lists[c[2]][c[3]])  # noqa: E731
    fwd = sig(lswap["forward"])
    a_, i, b, j = lswap["forward"]
    lists[a_][i], lists[b][j] = lists[b][j], lists[a_][i]
    assert fwd.move_id == fwd.undo_move_id == sig(lswap["reverse_same_coordinates"]).move_id == sig(lswap["reverse_flipped_coordinates"]).move_id
    assert [v for _, v in fwd.value_tokens] == [30, 2] and [e for _, e in fwd.entity_tokens] == [0, 1]


# ---- the edge scripts: what each must reach, judged on the mirror alone ---------------------------------------------------------------
def _decisions(results):
    return [(op[3], res, reasons, state) for op, res, reasons, state in results if op[0] == "is_accepted"]


def _check_tenure_1(s, results):
    assert tm.normalize_policy(s["policy"])[:4] == (1, 1, 1, 1)
    d = _decisions(results)
    assert [(n, r) for n, _, r, _ in d[:4]] == [("pe", {"entity"}), ("pv", {"value"}), ("pm", {"move"}), ("pu", {"undo"})]
    assert all(res is True and not r for _, res, r, _ in d[4:]) and len(d) == 8


def _check_two_tokens(s, results):
    assert len(s["sigs"]["s"].entity_tokens) == len(s["sigs"]["s"].value_tokens) == 2
    assert [(n, res) for n, res, _, _ in _decisions(results)] == [("e1", True), ("e2", False), ("v3", True), ("v4", False)]


def _check_entity_twice(s, results):
    a = tm.TabuSearch(s["policy"])
    a.phase_started([-10])
    for n in "abc":
        a.step_ended([-9], s["sigs"][n])
    assert [e for _, e in a.mem["entity"].entries] == [1, 1, 2]  # two slots
    assert [res for _, res, _, _ in _decisions(results)] == [False, False, True]
    states = [st for op, _, _, st in results if op[0] == "step_ended"]
    assert [sum(e == 1 for _, e in st[2]) for st in states] == [1, 1, 1, 1, 0]  # one evicted slot leaves it tabu


def _check_eviction(s, results):
    d = _decisions(results)
    assert d[0][3][1][0] == 3 == s["policy"][0] and d[0][3][1][2] == 3 == s["policy"][2]  # exactly `tenure` pushes: still held
    assert [res for _, res, _, _ in d] == [False, False, True, True] and d[2][3][1][0] == 4


def _check_never_recorded(s, results):
    d = _decisions(results)
    assert all(p < t for p, t in zip(d[1][3][1], s["policy"][:4]))  # fewer pushes than the tenure in every memory
    assert d[0][3][1] == (0, 0, 0, 0) and [res for _, res, _, _ in d] == [True, True, True, False]


def _check_ring_wraps(s, results):
    final = results[-1][3]
    assert final[1][2] >= 3 * s["policy"][2] and final[4] == [(6,), (7,)]


def _check_undo_then_move(s, results):
    assert [(n, res, r) for n, res, r, _ in _decisions(results)] == [("yx", False, {"undo"}), ("xy", False, {"move"}), ("other", True, set())]


def _check_swap_both(s, results):
    assert [(res, r) for _, res, r, _ in _decisions(results)] == [(False, {"move", "undo"})]


def _check_to_none(s, results):
    assert s["sigs"]["unassign"].value_tokens == [(tm.S, None)] and s["sigs"]["unassign"].move_id[-1] is None
    assert [(res, r) for _, res, r, _ in _decisions(results)] == [(False, {"value"}), (True, set())]


def _check_intra_list(s, results):
    intra = s["sigs"]["intra"]
    assert intra.entity_tokens == [(tm.S, 0)] and intra.move_id == (0, "x", 0, 1, 0, 2, 7) and intra.undo_move_id == (0, "x", 0, 2, 0, 1, 7)
    assert len(s["sigs"]["from0"].entity_tokens) == 2
    assert [(res, r) for _, res, r, _ in _decisions(results)] == [(False, {"entity"}), (True, set()), (False, {"entity", "move"})]


def _check_four_levels(s, results):
    assert s["levels"] == 4
    d = [op for op, _, _, _ in results if op[0] == "is_accepted"]
    best = tuple(results[1][3][0])
    assert tuple(d[0][2]) == best and d[0][4] is False and tuple(d[1][2])[:3] == best[:3] and d[1][2][3] == best[3] + 1 and d[1][4] is True


def _check_aspiration_off(s, results):
    (_, res, reasons, state), = _decisions(results)
    assert s["policy"][4] is False and res is False and reasons == {"entity"} and (1000,) > state[0]


def _check_best_unchanged(s, results):
    bests = [st[0] for op, _, _, st in results if op[0] in ("phase_started", "step_ended")]
    assert bests == [(-10,), (-10,), (-10,), (-8,), (-8,)]  # equal score; worse score without a move; a better one without a move; equal again
    assert [op[2] for op, _, _, _ in results if op[0] == "step_ended"] == ["a", None, None, None]


def _check_two_scopes(s, results):
    x, y = s["sigs"]["in_x"], s["sigs"]["in_y"]
    assert [e for _, e in x.entity_tokens] == [e for _, e in y.entity_tokens] and x.move_id[2:] == y.move_id[2:] and x.scope != y.scope
    assert [(n, res) for n, res, _, _ in _decisions(results)] == [("in_y", True), ("back_in_y", True), ("in_x", False)]


def _check_all_absent(s, results):
    assert s["policy"][:4] == [None, None, None, None] and tm.TabuSearch(s["policy"]).tenures == (None, None, 10, None)
    assert [(n, res) for n, res, _, _ in _decisions(results)] == [("m1", False), ("m12", True), ("m1", True), ("m2", False)]
    assert results[-1][3][1] == (0, 0, 11, 0)


EDGE_CHECKS = {
    "tenure_1_each_memory": _check_tenure_1, "two_tokens_tenure_1": _check_two_tokens, "entity_twice_two_slots": _check_entity_twice,
    "eviction_at_exactly_tenure": _check_eviction, "never_recorded_below_tenure": _check_never_recorded, "move_ring_wraps_three_times": _check_ring_wraps,
    "undo_alone_then_move_alone": _check_undo_then_move, "swap_refused_by_both": _check_swap_both, "to_none": _check_to_none,
    "intra_list_change_one_entity": _check_intra_list, "four_levels_equal_not_aspirational": _check_four_levels, "aspiration_off": _check_aspiration_off,
    "best_unchanged_by_equal_and_empty_steps": _check_best_unchanged, "same_id_two_scopes": _check_two_scopes, "all_absent_is_move_only_10": _check_all_absent,
}


def test_edge_scripts_cover_the_list():
    assert sorted(EDGE_CHECKS) == sorted(s["name"] for s in tm.EDGE_SCRIPTS) and len(EDGE_CHECKS) == 15


@pytest.mark.parametrize("script", tm.EDGE_SCRIPTS, ids=lambda s: s["name"])
def test_edge_scripts_reach_their_edges(script):
    EDGE_CHECKS[script["name"]](script, tm.run(script))


# ---- the stamp-table formulation ------------------------------------------------------------------------------------------------------
def test_stamp_table_is_the_fifo():
    """tabu(token) <=> stamp != 0 and pushes - stamp < tenure, against TabuMemory: 2,400 random sequences of pushes (single and
    record_many pairs, duplicates included) and queries, tenures 1..5 over 6 tokens, every token queried after every push."""
    rng = random.Random(20260101)
    n_seq = queries = 0
    for tenure in range(1, 6):
        for _ in range(480):
            fifo, stamps = tm.TabuMemory(tenure), tm.StampMemory(tenure)
            for _ in range(rng.randrange(1, 25)):
                for tok in [rng.randrange(6) for _ in range(rng.choice((1, 1, 2)))]:  # record / record_many
                    fifo.record(tok)
                    stamps.record(tok)
                for tok in range(6):
                    assert fifo.contains(tok) == stamps.contains(tok), (tenure, fifo.entries, stamps.stamp, tok)
                    queries += 1
                assert fifo.pushes == stamps.pushes and len(fifo.entries) == min(tenure, fifo.pushes)
            n_seq += 1
    assert n_seq >= 2000 and queries > 100000
    absent = tm.StampMemory(None)
    absent.record(1)
    assert not absent.contains(1) and absent.pushes == 0


# ---- the device packing ---------------------------------------------------------------------------------------------------------------
def test_model_packing_is_injective():
    """Every distinct identity / token of a small two-scope universe packs to a distinct word pair / index, equal ones to equal ones."""
    sx, sy = (0, "x"), (1, "y")
    pk = tm.ModelPacker({sx: (0, 0, 0), sy: (1, 4, 4)})  # 4 entities and values None, 0..2 under x; lists under y
    sigs = []
    for e, f, t in itertools.product(range(4), (None, 0, 1, 2), (None, 0, 1, 2)):
        sigs.append(tm.change_signature(sx, e, f, t))
    for l, r in itertools.permutations(range(4), 2):
        sigs.append(tm.swap_signature(sx, l, r, 0, 1))
    for a, i, b, j, v in itertools.product(range(2), range(3), range(2), range(3), range(2)):
        sigs.append(tm.list_change_signature(sy, a, i, b, j, v))
        sigs.append(tm.list_swap_signature(sy, a, i, v, b, j, 1 - v))
    ids = {}
    for s in sigs:
        for t in (s.move_id, s.undo_move_id):
            assert ids.setdefault(pk.identity(t), t) == t, (t, ids[pk.identity(t)])
    assert len(ids) == len({t for s in sigs for t in (s.move_id, s.undo_move_id)})
    toks = {}
    for s in sigs:
        for t in s.entity_tokens:
            assert toks.setdefault(("e", pk.entity(t)), t) == t
        for t in s.value_tokens:
            assert toks.setdefault(("v", pk.value(t)), t) == t
    assert pk.value((sx, None)) == 0 and pk.value((sx, 2)) == 3 and pk.value((sy, 0)) == 5 and pk.entity((sy, 1)) == 5
    packed = pk.sig(tm.list_change_signature(sy, 0, 1, 0, 3, 1))
    assert packed["entity"] == [4, tm.NO_TOKEN] and packed["value"] == [6, tm.NO_TOKEN]
    assert packed["move_id"] == ((3 << 56) | (1 << 48) | (0 << 24) | 1, (0 << 48) | (2 << 24) | 2)


@pytest.mark.parametrize("script", tm.all_scripts(), ids=lambda s: s["name"])
def test_device_plan_straddles_the_rule(script):
    """What the GPU script test sends: 64 candidates per decide record, masked lanes never accepted; over the records of a script both
    outcomes occur unless the script's memories are empty throughout, and where a memory holds an entry a candidate that only it refuses
    is among them."""
    plan, packer = tm.device_plan(script)
    assert plan[0]["op"] == tm.OP_PHASE_STARTED
    decides = [r for r in plan if r["op"] == tm.OP_DECIDE]
    if script.get("requires_move_signatures"):
        assert not decides
        return
    assert decides
    for rec in decides:
        assert len(rec["cands"]) == 64
        for lane in tm.MASKED_LANES:
            assert not (rec["accept"] >> lane) & 1
        live = [k for k, n in zip(tm.MEMORIES, (len(rec["state"][2]), len(rec["state"][3]), len(rec["state"][4]), len(rec["state"][5]))) if n]
        for k in live:
            assert any(k in reasons for reasons, _ in rec["kinds"]), (script["name"], k)
        assert any(not reasons for reasons, _ in rec["kinds"])
        if live:
            assert 0 < bin(rec["accept"]).count("1") < 64 - len(tm.MASKED_LANES)
    kinds = set().union(*(r["kinds"] for r in decides))
    assert any(above for _, above in kinds) and any(not above for _, above in kinds)  # scores on both sides of the acceptor's best
