"""CPU test of the oracle's CVRP model with per-constraint weights (oracle/sfo_models.hpp: make_cvrp w_assigned / w_cap / w_dist --
the checker the GPU tests of the 32-bit weight bounds need).  Scores and the per-constraint rows against a numpy recomputation;
with one weight w on all three constraints a LateAcceptance + AcceptedCount run follows the unweighted run step for step (positive
uniform scaling keeps the order of every score) with every score multiplied by w."""
import numpy as np
import pytest

DEFAULT_BITS = 16 | 32 | 128 | 256 | 64 | 512 | 1024  # the seven leaves of the default list policy


def _problem(seed, n, v, cap, drop=()):
    from solverforge_amd import datasets

    p = datasets.make_cvrp(n, v, cap, seed=seed)
    p["routes"] = [[c for c in rt if c not in drop] for rt in p["routes"]]  # dropped customers stay unassigned
    return p


def _numpy_parts(p, w):
    m, dem, depot, cap = p["matrix"], p["demands"].astype(np.int64), p["depot"], p["capacity"]
    dist = over = 0
    for rt in p["routes"]:
        if rt:
            path = [depot] + list(rt) + [depot]
            dist += int(m[path[:-1], path[1:]].sum())
            over += max(0, int(dem[list(rt)].sum()) - cap)
    unassigned = len(set(int(c) for c in p["customers"]) - {c for rt in p["routes"] for c in rt})
    return np.array([-w[0] * unassigned, -w[1] * over, -w[2] * dist]), (unassigned, over, dist)


def _oracle(oracle, p, weights):
    return oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"], weights=weights)


@pytest.mark.parametrize("seed,n,v,cap,drop,weights", [
    (1, 40, 5, 30, (), (1, 1, 1)),
    (2, 60, 4, 25, (3, 17), (7, 1, 1)),
    (3, 50, 6, 20, (5,), (3, 1000, 13)),
    (4, 80, 3, 60, (1, 2, 40), (1 << 20, 1 << 9, 37)),
    (5, 30, 2, 10, (), (1, (1 << 40) + 3, 1 << 30)),
])
def test_weighted_scores_against_numpy(oracle, seed, n, v, cap, drop, weights):
    p = _problem(seed, n, v, cap, drop)
    o = _oracle(oracle, p, weights)
    parts, raw = _numpy_parts(p, weights)
    assert raw[1] > 0, "the problem should overload some route"
    want = np.array([parts[0] + parts[1], parts[2]])
    assert (o.score()[:2] == want).all(), (o.score(), want)
    assert (o.fresh_score()[:2] == want).all()
    sc, cnt = o.evaluate_each()
    assert len(sc) == 3
    assert sc[0, 0] == parts[0] and sc[0, 1] == 0
    assert sc[1, 0] == parts[1] and sc[1, 1] == 0
    assert sc[2, 0] == 0 and sc[2, 1] == parts[2]
    # the unweighted model's rows scaled
    sc1, cnt1 = _oracle(oracle, p, (1, 1, 1)).evaluate_each()
    assert (cnt == cnt1).all()
    for k in range(3):
        assert (sc[k] == sc1[k] * weights[k]).all()


@pytest.mark.parametrize("w", [3, 1 << 16])
def test_uniform_weight_follows_the_unweighted_trajectory(oracle, w):
    p = _problem(6, 45, 5, 35, drop=(9,))
    runs = []
    for weights in ((1, 1, 1), (w, w, w)):
        o = _oracle(oracle, p, weights)
        o.configure(leaves=DEFAULT_BITS, random_seed=4, max_nearby=10, la_size=400, limit=256)
        o.set_ruin(2, 5, 10, variable_name="visits")
        o.phase_start()
        runs.append(o)
    a, b = runs
    for step in range(40):
        a.steps(1)
        b.steps(1)
        assert a.get_lists(0) == b.get_lists(0), step
        assert (b.score()[:2] == a.score()[:2] * w).all(), step
        assert (b.best_score()[:2] == a.best_score()[:2] * w).all(), step
    assert a.stats() == b.stats()
    assert a.stats()["moves_applied"] > 10
    assert (b.fresh_score()[:2] == b.score()[:2]).all()
