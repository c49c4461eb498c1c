"""CPU tests of datasets.make_cvrptw and of the parity cases tests/test_gpu_kopt_time_windows.py runs on it, with the oracle alone.

A mode-2 parity case can only tell the complete hook from "no hook" and from "refuse everything" when the oracle's mode-2 run accepts
at least one reversal AND ends with lists that differ from its mode-0 run on the same data (so at least one improving reversal was
refused by a window).  That is a condition on the inputs, asserted here for every committed case and sweep bound; a case that misses
it gets another seed or slack, the condition stays."""
import numpy as np
import pytest

BIG = 10**6  # capacity out of the way: the windows alone decide


def _family(slack):
    return [
        ("plain-60/6", dict(n_customers=60, n_vehicles=6, capacity=BIG, seed=3, slack=slack, tw_seed=1)),
        ("ragged-130/9", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2)),
        ("one-route-130", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2, one_route=True)),
        ("one-route-130-lo=arrival", dict(n_customers=130, n_vehicles=9, capacity=BIG, seed=21, slack=slack, tw_seed=2, one_route=True, lo_slack=0)),
    ]


# the same list as tests/test_gpu_kopt_time_windows.py::PARITY_CASES
PARITY_CASES = [c for s in (300, 1000, 3000) for c in _family(s)] + [
    ("cvrp-1000/100-cap55", dict(n_customers=1000, n_vehicles=100, capacity=55, seed=0, slack=s, tw_seed=3)) for s in (1000, 3000)]
IDS = [f"{name}-slack{kw['slack']}" for name, kw in PARITY_CASES]


def _oracle_model(oracle, p):
    m = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    lo, hi = p["time_windows"]
    m.set_time_windows(lo, hi, p["service"], p["travel"], p["departure"])
    return m


def test_make_cvrptw_is_deterministic_and_extends_make_cvrp():
    from solverforge_amd import datasets

    kw = dict(n_customers=130, n_vehicles=9, capacity=90, seed=21, slack=1000, tw_seed=2)
    a, b = datasets.make_cvrptw(**kw), datasets.make_cvrptw(**kw)
    base = datasets.make_cvrp(130, 9, 90, seed=21)
    for k in ("matrix", "demands", "customers"):
        assert (a[k] == base[k]).all()
    assert a["routes"] == base["routes"] and a["capacity"] == base["capacity"] and a["depot"] == base["depot"]
    for k in ("service", "travel"):
        assert (a[k] == b[k]).all() and a[k].dtype == np.int64
    assert all((x == y).all() for x, y in zip(a["time_windows"], b["time_windows"])) and a["departure"] == b["departure"] == 0
    assert (a["travel"] == a["matrix"]).all() and a["travel"] is not a["matrix"]
    assert a["service"][0] == 0 and a["service"].min() >= 0 and a["service"].max() <= 5 and len(set(a["service"].tolist())) == 6
    lo, hi = a["time_windows"]
    assert (lo >= 0).all() and (lo <= hi).all()
    c = datasets.make_cvrptw(**dict(kw, tw_seed=3))
    assert not (c["service"] == a["service"]).all() and not (c["time_windows"][1] == hi).all()
    one = datasets.make_cvrptw(**dict(kw, one_route=True))
    assert one["routes"][0] == list(range(1, 131)) and all(rt == [] for rt in one["routes"][1:])


def test_lo_slack_zero_opens_every_window_at_the_start_routes_arrival():
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(n_customers=40, n_vehicles=4, capacity=BIG, seed=7, slack=500, tw_seed=9, lo_slack=0, departure=17)
    lo, hi = p["time_windows"]
    for rt in p["routes"]:
        t, prev = 17, 0
        for v in rt:
            t += int(p["travel"][prev, v])
            assert lo[v] == t  # no waiting on the start route, and none to spare
            t += int(p["service"][v])
            assert t <= hi[v] <= t + 500
            prev = v


@pytest.mark.parametrize("name,kw", PARITY_CASES, ids=IDS)
def test_capacity_feasible_start_routes_are_time_feasible(oracle, name, kw):
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(**kw)
    m = _oracle_model(oracle, p)
    n_ok = 0
    for rt in p["routes"]:
        if sum(int(p["demands"][c]) for c in rt) <= p["capacity"]:
            assert m.route_feasible(rt), rt
            n_ok += 1
    assert n_ok > 0


@pytest.mark.parametrize("max_sweeps", [1000, 3])
@pytest.mark.parametrize("name,kw", PARITY_CASES, ids=IDS)
def test_parity_cases_tell_mode_2_from_mode_0_and_from_refuse_everything(oracle, name, kw, max_sweeps):
    from solverforge_amd import datasets

    p = datasets.make_cvrptw(**kw)
    res = {}
    for mode in (0, 2):
        m = _oracle_model(oracle, p)
        st = m.construct_list_k_opt(2, mode, max_sweeps)
        res[mode] = (m.get_lists(0), int(st[1]))
    assert res[2][1] >= 1, "the oracle's mode-2 run accepts nothing"
    assert res[2][0] != res[0][0], "no improving reversal was refused by a window"
