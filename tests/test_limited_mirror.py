"""CPU: tests/limited_mirror.py -- the reference's limited-cursor test as data, the pin of the mirror's union scheduler and step rule on the
oracle's own (no budgets: the mirror must be the oracle, pull for pull), and the edges the scripts of tests/limited_cases.py must reach on
the mirror so that the GPU tests, which run the same scripts, cannot pass vacuously."""
import numpy as np
import pytest

import limited_cases as lc
import limited_mirror as lm

_memo = {}


def _rec(mv):
    return tuple(int(x) for x in mv.tolist())


# ---- 1. the reference's test as data ----------------------------------------------------------------------------------------------------
def test_reference_limited_cursor_cases():
    cases = lm.golden_file()["cases"]
    assert any(c["inner_total"] == 100 and c["limit"] == 3 and c["pulls"] == 3 and c["inner_generated"] == 3 for c in cases)
    assert any(c["limit"] == 0 for c in cases) and any(c["limit"] >= c["inner_total"] > 0 for c in cases)
    for c in cases:
        out, generated = lm.limited(range(c["inner_total"]), c["limit"])
        assert out == list(range(c["pulls"])) and generated == c["inner_generated"], c["name"]  # a prefix; the inner cursor is not touched after it


# ---- 2. the pin ---------------------------------------------------------------------------------------------------------------------------
PIN_UNIONS = {  # model -> unions of 2, 3 and 4 leaves in the oracle's child order
    "cvrp": (("list_change", "list_swap"), ("list_change", "list_swap", "list_reverse"), ("list_change", "list_swap", "sublist_change", "list_reverse")),
    "colouring": (("change", "swap"),),
    "jobshop": (("list_change", "change"), ("list_swap", "change", "swap"), ("list_change", "list_swap", "change", "swap")),
}
PIN_WEIGHTS = {2: ((3, 1), (0, 2)), 3: ((1, 4, 2), (2, 0, 1)), 4: ((2, 1, 3, 1), (1, 0, 5, 2))}


@pytest.mark.parametrize("model", sorted(PIN_UNIONS))
def test_union_stream_is_the_oracles(oracle, model):
    checked = 0
    for leaves in PIN_UNIONS[model]:
        script = {"model": model, "leaves": leaves}
        bits = lc.leaf_bits(script)
        kinds = None
        for order in lm.ORDERS:
            for weights in (None,) + (PIN_WEIGHTS[len(leaves)] if order in (lm.RANDOM, lm.STRATIFIED_RANDOM) else ()):
                o = lc.oracle_model(oracle, script, union_order=order, weights=weights)
                for step_index, seed in ((0, 1), (3, 0x9E3779B97F4A7C15), (17, 12345)):
                    for sel_order in (0, 3):
                        children = [o.enumerate(b, step_index, seed, sel_order) for b in bits]
                        if kinds is None:  # every child's records are of a kind of its own: equal records name the same child
                            kinds = [set(c["kind"].tolist()) for c in children]
                            assert all(len(k) == 1 for k in kinds) and len(set(map(tuple, kinds))) == len(kinds)
                        pulls = lm.union_stream(oracle, [len(c) for c in children], order, step_index, seed, weights)
                        theirs = o.enumerate(0, step_index, seed, sel_order)
                        assert len(pulls) == len(theirs) == sum(len(c) for c, w in zip(children, weights or [1] * len(children)) if w)
                        assert [_rec(children[c][i]) for c, i in pulls] == [_rec(m) for m in theirs], (leaves, order, weights, step_index)
                        assert all(int(m["kind"]) in kinds[c] for (c, _), m in zip(pulls, theirs))
                        checked += 1
    assert checked >= 30


@pytest.mark.parametrize("model", sorted(PIN_UNIONS))
@pytest.mark.parametrize("acceptor,forager", lc.CONFIGS)
def test_unlimited_step_mirror_is_the_oracles_traced_step(oracle, model, acceptor, forager):
    script = dict(lc._s(model, lm.STRATIFIED_RANDOM))
    o2, mirror = lc.search_mirror(oracle, script, lc.SEED, acceptor, forager)
    o = lc.oracle_model(oracle, script)
    o.configure(acceptor=acceptor, la_size=lc.LA_SIZE, forager=forager, limit=lc.ACCEPTED_LIMIT, random_ties=False, selection_order=lc.ORDER_RANDOM,
                leaves=sum(lc.leaf_bits(script)), random_seed=lc.SEED)
    o.set_sublist_sizes(*lc.SUBLIST_SIZES)
    o.phase_start()
    for step in range(20):
        om, osc, of, oap, omv = o.step_traced()
        rec = mirror.step()
        cands = rec["candidates"][:rec["consumed"]]
        assert [c["record"] for c in cands] == [_rec(m) for m in om], (model, step)
        assert [c["doable"] for c in cands] == ((of & 1) != 0).tolist() and rec["accepted"] == ((of & 2) != 0).tolist(), (model, step)
        assert oap == (rec["pick"] is not None) and (not oap or _rec(omv) == cands[rec["pick"]]["record"]), (model, step)
        assert tuple(int(x) for x in o.score()[:2]) == rec["score"], (model, step)
    assert o.stats() == {k: mirror.stats[k] for k in lm.COUNTERS}
    assert lc.state_of(o, script) == lc.state_of(o2, script)


# ---- 3. the scripts reach the edges ---------------------------------------------------------------------------------------------------
def _search(oracle, name):
    """records[(acceptor, forager)] = the first STEPS steps of the script on the mirror."""
    if name not in _memo:
        out = {}
        for cfg in lc.CONFIGS:
            _, mirror = lc.search_mirror(oracle, lc.SEARCH[name], lc.SEED, *cfg)
            out[cfg] = [mirror.step() for _ in range(lc.STEPS)]
        _memo[name] = out
    return _memo[name]


def _vnd(oracle, name):
    if name not in _memo:
        _, ph = lc.vnd_mirror(oracle, lc.VND[name], lc.SEED)
        _memo[name] = (ph.run(lc.VND[name]["steps"]), ph)
    return _memo[name]


def _pulled(rec, n):
    kids = [c["child"] for c in rec["candidates"]]
    return [kids.count(c) for c in range(n)]


def _all_records(oracle, name):
    return [rec for recs in _search(oracle, name).values() for rec in recs]


def test_child_limits_bind_at_their_sizes(oracle):
    for name, child, limit in (("colouring_child_63", 1, 63), ("colouring_child_64", 0, 64), ("cvrp_child_65", 0, 65), ("cvrp_child_128", 1, 128),
                               ("colouring_child_129", 1, 129), ("jobshop_zero_one", 0, 0), ("jobshop_zero_one", 1, 1)):
        s = lc.SEARCH[name]
        assert s["child"][child] == limit
        for rec in _all_records(oracle, name):
            assert rec["lengths"][child] > (130 if limit >= 63 else 1), name  # the unlimited cursor is longer
            assert _pulled(rec, len(s["leaves"]))[child] == limit, name
            assert [c["index"] for c in rec["candidates"] if c["child"] == child] == list(range(limit)), name  # a prefix of the child's cursor
    assert {lc.SEARCH[n]["order"] for n in ("colouring_child_63", "colouring_child_64", "cvrp_child_65", "cvrp_child_128", "colouring_child_129")} == set(lm.ORDERS)


def test_a_stratified_child_is_cut_inside_a_cycle_and_at_a_cycles_end(oracle):
    seen = set()
    for name, s in lc.SEARCH.items():
        if s["order"] != lm.STRATIFIED_RANDOM or s["weights"] is not None or s["root"] is not None:
            continue
        n = len(s["leaves"])
        for rec in _all_records(oracle, name):
            kids = [c["child"] for c in rec["candidates"]]
            for child, limit in s["child"].items():
                if not 0 < limit < rec["lengths"][child]:
                    continue
                last = max(i for i, c in enumerate(kids) if c == child)
                live = [c for c in range(n) if s["child"].get(c) != 0]
                if any(kids[:last].count(c) >= min(rec["lengths"][c], s["child"].get(c, 1 << 40)) for c in live if c != child):
                    continue  # another child ended before: the cycles are no longer aligned with the start of the stream
                seen.add("end" if last % len(live) == len(live) - 1 else "inside")
    assert seen == {"end", "inside"}


def test_a_child_is_cut_in_the_step_in_which_another_runs_dry(oracle):
    s = lc.SEARCH["jobshop_cut_and_dry"]
    for rec in _all_records(oracle, "jobshop_cut_and_dry"):
        pulled = _pulled(rec, 4)
        assert pulled[0] == 30 < rec["lengths"][0] and pulled[2] == 40 < rec["lengths"][2]  # cut
        assert pulled[1] == rec["lengths"][1] and pulled[3] == rec["lengths"][3] and 1 not in s["child"]  # ran dry by themselves
        kids = [c["child"] for c in rec["candidates"]]
        assert max(i for i, c in enumerate(kids) if c == 1) < max(i for i, c in enumerate(kids) if c == 0)  # list swap (some 23) ends before the cut binds
    w = lc.SEARCH["jobshop_cut_weighted"]
    for rec in _all_records(oracle, "jobshop_cut_weighted"):
        assert _pulled(rec, 4)[2] == 0 and _pulled(rec, 4)[3] == 17 and w["weights"][2] == 0


def test_a_limit_above_the_cursors_length_is_the_identity(oracle):
    s = lc.SEARCH["jobshop_identity"]
    free = dict(s, child={})
    for cfg in lc.CONFIGS:
        _, a = lc.search_mirror(oracle, s, lc.SEED, *cfg)
        _, b = lc.search_mirror(oracle, free, lc.SEED, *cfg)
        for _ in range(lc.STEPS):
            ra, rb = a.step(), b.step()
            assert s["child"][0] > ra["lengths"][0] and s["child"][3] >= ra["lengths"][3]
            assert [c["record"] for c in ra["candidates"]] == [c["record"] for c in rb["candidates"]] and ra["pick"] == rb["pick"] and ra["score"] == rb["score"]


def test_every_child_at_zero_is_an_empty_step(oracle):
    for cfg, recs in _search(oracle, "colouring_all_zero").items():
        assert all(rec["candidates"] == [] and rec["consumed"] == 0 and rec["pick"] is None and min(rec["lengths"]) > 0 for rec in recs)
        assert len({rec["score"] for rec in recs}) == 1 and [rec["step_index"] for rec in recs] == list(range(lc.STEPS))  # the steps count, nothing moves


def test_root_limits_bind_at_their_sizes(oracle):
    cut_inside = cut_at_end = False
    for name, root in (("jobshop_root_1", 1), ("cvrp_root_63", 63), ("colouring_root_64", 64), ("cvrp_root_65", 65), ("colouring_root_129", 129)):
        s = lc.SEARCH[name]
        assert s["root"] == root and not s["child"]
        for rec in _all_records(oracle, name):
            assert len(rec["candidates"]) == root < sum(rec["lengths"]) and min(rec["lengths"]) * len(rec["lengths"]) > root, name  # no child ran dry
            if s["order"] == lm.STRATIFIED_RANDOM:
                cut_inside = cut_inside or root % len(s["leaves"]) != 0
                cut_at_end = cut_at_end or root % len(s["leaves"]) == 0
    assert cut_inside and cut_at_end  # a whole-cycles batch that keeps a partial cycle, and one that does not


def test_root_and_child_limits_bind_in_both_orders(oracle):
    for rec in _all_records(oracle, "colouring_child_then_root"):
        kids = [c["child"] for c in rec["candidates"]]
        assert len(kids) == 100 and kids.count(1) == 10 and max(i for i, c in enumerate(kids) if c == 1) < 99  # the child's first, the root's later
    for rec in _all_records(oracle, "cvrp_root_before_child"):
        kids = [c["child"] for c in rec["candidates"]]
        assert len(kids) == 64 and 0 < kids.count(0) < 60  # the root's ends the step; the child's never binds


def test_a_forager_quits_before_any_limit_binds(oracle):
    hits = 0
    for name, s in lc.SEARCH.items():
        for (acceptor, forager), recs in _search(oracle, name).items():
            for rec in recs:
                kids = [c["child"] for c in rec["candidates"][:rec["consumed"]]]
                if forager == lc.ACCEPTED_COUNT and rec["consumed"] < len(rec["candidates"]) and (s["child"] or s["root"] is not None):
                    assert sum(rec["accepted"]) == lc.ACCEPTED_LIMIT
                    if all(kids.count(c) < lim for c, lim in s["child"].items()) and (s["root"] is None or len(kids) < s["root"]):
                        hits += 1
    assert hits >= 3


def test_vnd_cut_just_inside_and_just_outside(oracle):
    inside, _ = _vnd(oracle, "cvrp_inside")
    outside, _ = _vnd(oracle, "cvrp_outside")
    s = lc.VND["cvrp_inside"]
    o = lc.oracle_model(oracle, s)
    full = o.enumerate(lc.leaf_bits(s)[0], 0, oracle.lib().sfo_step_seed(lc.SEED, 0), 0)
    sc, dv = o.evaluate_moves(full)
    cur = tuple(int(x) for x in o.score()[:2])
    improving = [i for i, (row, ok) in enumerate(zip(sc, dv)) if ok and tuple(int(x) for x in row[:2]) > cur]
    assert improving[0] == 3 and s["limits"][0] == 4 and lc.VND["cvrp_outside"]["limits"][0] == 3
    assert inside[0]["k"] == 0 and inside[0]["cursor"] == 4 and inside[0]["pick"] == 3 and inside[1]["k"] == 0  # the last candidate inside the cut
    assert outside[0]["k"] == 0 and outside[0]["cursor"] == 3 and outside[0]["pick"] is None and outside[1]["k"] == 1  # idle: k += 1
    assert any(rec["k"] == 1 and rec["pick"] is not None for rec in outside)  # the union behind it finds what the cut hid


def test_vnd_union_neighbourhoods(oracle):
    seq, ph_seq = _vnd(oracle, "cvrp_union_sequential")
    strat, ph_strat = _vnd(oracle, "cvrp_union_stratified")
    members = lc.hoods(lc.VND["cvrp_union_sequential"])[0][0]
    assert any(rec["k"] == 0 and rec["pick"] is not None and rec["children"][rec["pick"]] == members[1] for rec in seq)  # the pick is the second child's
    # the two orders pull the same candidates in another order: they part where equal bests lie in both children
    parted = None
    for a, b in zip(seq, strat):
        assert a["k"] == b["k"] and sorted(map(_rec, a["moves"])) == sorted(map(_rec, b["moves"]))
        if a["pick"] is not None and _rec(a["moves"][a["pick"]]) != _rec(b["moves"][b["pick"]]):
            parted = (a, b)
            break
    assert parted is not None
    a, b = parted
    assert a["k"] == 0 and a["ties"] >= 2 and a["ties"] == b["ties"] and a["score"] == b["score"]
    assert a["children"][a["pick"]] != b["children"][b["pick"]]
    assert a["children"] == sorted(a["children"]) and b["children"][:4] in ([0, 1, 0, 1], [1, 0, 1, 0])  # Sequential drains, StratifiedRandom alternates
    assert ph_seq.done and ph_seq.k == ph_seq.n == 2 and ph_strat.done  # the descent ends at k == the number of neighbourhoods


def test_vnd_group_of_three_draws_offset_and_stride_over_three(oracle):
    recs, ph = _vnd(oracle, "jobshop_three")
    group = [rec for rec in recs if rec["k"] == 1]
    assert group and all(set(rec["children"]) <= {1, 2, 3} for rec in group)
    assert any(rec["offset_stride"][0] != rec["offset_stride"][1] for rec in group)  # (offset, stride) over 3 children is not that over 4 leaves
    assert all(rec["children"].count(3) == 25 for rec in group)  # the per-leaf limit applies inside the group
    assert all(rec["cursor"] == 20 for rec in recs if rec["k"] == 0)  # the limit around the one-leaf neighbourhood
    assert ph.done and ph.k == ph.n == 2


def test_vnd_other_orders_run_to_their_end(oracle):
    for name in ("colouring_random", "jobshop_round_robin"):
        recs, ph = _vnd(oracle, name)
        s = lc.VND[name]
        assert ph.done and ph.k == ph.n == len(s["groups"]) and recs[-1]["pick"] is None
        for rec in recs:
            members, _, limit = lc.hoods(s)[rec["k"]]
            assert set(rec["children"]) <= set(members) and (limit is None or rec["cursor"] <= limit)
        assert any(rec["cursor"] == lim for rec in recs for lim in [lc.hoods(s)[rec["k"]][2]] if lim is not None)  # a neighbourhood limit binds
    assert any(rec["pick"] is not None and len(lc.hoods(lc.VND["jobshop_round_robin"])[rec["k"]][0]) == 2 for rec in _vnd(oracle, "jobshop_round_robin")[0])
