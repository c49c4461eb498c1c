"""CPU: tests/acceptor_mirror.py (GreatDeluge, StepCountingHillClimbing restated) over the reference's own unit tests
(tests/golden/acceptor_goldens.json: call sequences and expected results as data) and over the hand-written edge scripts, each of which
must reach the edge it is named for.  The GPU tests compare the device with this mirror, so it is pinned here without a device."""
import pytest

import acceptor_mirror as am


def test_goldens_are_the_eleven_reference_tests():
    g = am.goldens()
    assert len(g) == 11 and len({s["name"] for s in g}) == 11
    assert sum(s["acceptor"] == "great_deluge" for s in g) == 5 and sum(s["acceptor"] == "step_counting" for s in g) == 6
    for s in g:
        assert s["source"].startswith("crates/solverforge-solver/src/phase/localsearch/acceptor/") and s["levels"] == 1
        assert s["ops"][0][0] == "phase_started"


@pytest.mark.parametrize("script", am.goldens(), ids=lambda s: s["name"])
def test_mirror_passes_the_reference_tests(script):
    results = am.run(script)  # asserts every expected boolean / counter of the script
    assert sum(op[0] in ("is_accepted", "since") for op, _ in results) >= 1


def test_rounding_helpers():
    assert [am.round_half_away(v) for v in (0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, 2.4999999999999996)] == [1.0, -1.0, 2.0, 3.0, -3.0, 0.0, 2.0]
    assert am.f64_as_i64(float("nan")) == 0 and am.f64_as_i64(1e300) == am.I64_MAX and am.f64_as_i64(-1e300) == am.I64_MIN
    assert am.as_f64((1 << 53) + 1) == float(1 << 53) and am.as_f64((1 << 53) + 3) == float((1 << 53) + 4)  # ties to even
    assert am.wrap(am.I64_MAX + 1) == am.I64_MIN and am.wrap(-am.I64_MIN) == am.I64_MIN


@pytest.mark.parametrize("script", am.EDGE_SCRIPTS, ids=lambda s: s["name"])
def test_edge_scripts_reach_their_edges(script):
    results = am.run(script)
    expect = script["expect"]
    a = am.make(script)
    a.phase_started(script["ops"][0][1])
    if "increment" in expect:
        assert list(a.increment()) == expect["increment"]
    if "product" in expect:
        assert am.as_f64(a.abs0[0]) * a.rain_speed == expect["product"]
    if "water_above_cur" in expect:
        b, hit = am.make(script), False
        for op, res in results:
            if op[0] == "phase_started":
                b.phase_started(op[1])
            elif op[0] == "step_ended":
                b.step_ended(op[1])
            elif op[0] == "is_accepted" and tuple(op[1]) == tuple(op[2]) and b.water > tuple(op[1]):
                assert res is False
                hit = True
        assert hit
    if "since_max" in expect or "reset_at" in expect:
        b, seen, resets = am.make(script), [], []
        for op, _ in results:
            if op[0] == "phase_started":
                b.phase_started(op[1])
            elif op[0] == "step_ended":
                before = b.since
                b.step_ended(op[1])
                seen.append(b.since)
                if b.since == 0:
                    resets.append(before)
        assert max(seen) == expect["since_max"]
        if "reset_at" in expect:
            assert expect["reset_at"] in resets and expect["reset_at"] == b.limit - 1


def test_edge_scripts_cover_the_list():
    """Every edge the GPU script test is meant to carry is present, by what the scripts themselves contain."""
    by = {s["name"]: s for s in am.EDGE_SCRIPTS}
    assert by["half_negative_initial"]["ops"][0][1][0] < 0 < by["half_positive_initial"]["ops"][0][1][0]
    assert by["zero_initial"]["ops"][0][1] == [0] and by["zero_speed"]["param"] == 0.0 and by["negative_speed"]["param"] < 0 and by["tiny_speed"]["param"] == 1e-300
    four = by["four_levels_last_decides"]
    assert four["levels"] == 4 and all(op[1][:3] == op[2][:3] and op[1][3] != op[2][3] or op[1] == op[2] for op in four["ops"] if op[0] == "is_accepted")
    assert abs(by["initial_past_2_53"]["ops"][0][1][0]) >= (1 << 53) + 1
    assert [by[n]["param"] for n in ("limit_0", "limit_1", "limit_u64_max")] == [0, 1, (1 << 64) - 1]
    eq = by["equal_is_not_improved"]
    assert any(op[0] == "step_ended" and op[1] == eq["ops"][0][1] for op in eq["ops"])


@pytest.mark.parametrize("script", am.all_scripts(), ids=lambda s: s["name"])
def test_device_plan_straddles_the_threshold(script):
    """What the GPU test sends: 64 candidates per decide record; unless the rule admits no refusal (or no acceptance) at all there,
    both outcomes occur among them, and lanes that are not doable are never accepted."""
    plan = am.device_plan(script)
    assert plan[0]["op"] == am.OP_PHASE_STARTED
    for rec in plan:
        if rec["op"] != am.OP_DECIDE:
            continue
        assert len(rec["sc"]) == 64 and all(len(c) == 4 for c in rec["sc"])
        for lane in am.NOT_DOABLE_LANES:
            assert not (rec["accept"] >> lane) & 1
        n = bin(rec["accept"]).count("1")
        assert n > 0  # a candidate above the last step score is among them
        open_door = script["acceptor"] == "step_counting" and n == 64 - len(am.NOT_DOABLE_LANES)
        assert open_door or n < 64 - len(am.NOT_DOABLE_LANES)
