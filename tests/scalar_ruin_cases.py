"""The model scripts of the scalar ruin-and-recreate tests: a model, the leaf's parameters, the search around it, and how the oracle and
the device build it.  tests/test_scalar_ruin_mirror.py runs them on the mirror alone (they must reach the edges of the rule);
tests/test_gpu_scalar_ruin.py runs them on the device against the mirror."""
import numpy as np

import scalar_ruin_mirror as rm

HC, LA, BEST, COUNT = rm.HILL_CLIMBING, rm.LATE_ACCEPTANCE, rm.BEST_SCORE, rm.ACCEPTED_COUNT
ORIGINAL, RANDOM, SHUFFLED = rm.ORDER_ORIGINAL, rm.ORDER_RANDOM, rm.ORDER_SHUFFLED
FF, CI = rm.FIRST_FIT, rm.CHEAPEST_INSERTION
LA_SIZE, LIMIT = 5, 4

# name -> model, model arguments, leaf parameters, (acceptor, forager), selection order, traced steps, random seed
SCRIPTS = {
    "colouring_ff": dict(model="colouring", args=dict(n=60, e=140, k=3, seed=11), leaf=dict(recreate=FF), search=(HC, BEST), order=RANDOM, steps=12, seed=5),
    "colouring_ci": dict(model="colouring", args=dict(n=70, e=170, k=4, seed=12), leaf=dict(recreate=CI), search=(LA, COUNT), order=SHUFFLED, steps=12, seed=6),
    "colouring_original": dict(model="colouring", args=dict(n=40, e=100, k=3, seed=13), leaf=dict(recreate=CI, min_ruin_count=3, max_ruin_count=3, moves_per_step=6),
                               search=(LA, COUNT), order=ORIGINAL, steps=10, seed=7),
    "colouring_sparse_start": dict(model="colouring", args=dict(n=40, e=90, k=3, seed=14, assigned_every=9), leaf=dict(recreate=FF, min_ruin_count=1, max_ruin_count=3),
                                   search=(HC, BEST), order=RANDOM, steps=8, seed=8),
    "required_empty_list": dict(model="colouring", args=dict(n=40, e=90, k=3, seed=15, required=True, all_assigned=True, empty_lists_every=3),
                                leaf=dict(recreate=FF, min_ruin_count=1, max_ruin_count=3), search=(LA, COUNT), order=RANDOM, steps=8, seed=9),
    "required_limit_zero": dict(model="colouring", args=dict(n=40, e=90, k=3, seed=16, required=True, all_assigned=True),
                                leaf=dict(recreate=FF, value_candidate_limit=0), search=(HC, BEST), order=RANDOM, steps=3, seed=10),
    "three_entities": dict(model="colouring", args=dict(n=3, e=2, k=3, seed=17, all_assigned=True), leaf=dict(recreate=CI, min_ruin_count=2, max_ruin_count=5, moves_per_step=4),
                           search=(LA, COUNT), order=RANDOM, steps=8, seed=11),
    "wide_16x8": dict(model="colouring", args=dict(n=50, e=120, k=4, seed=18), leaf=dict(recreate=CI, min_ruin_count=8, max_ruin_count=8, moves_per_step=16),
                      search=(LA, COUNT), order=RANDOM, steps=8, seed=12),
    "one_move": dict(model="colouring", args=dict(n=50, e=120, k=4, seed=19), leaf=dict(recreate=FF, min_ruin_count=8, max_ruin_count=8, moves_per_step=1),
                     search=(HC, BEST), order=RANDOM, steps=8, seed=13),
    "assignment_range": dict(model="assignment", args=dict(lists=False), leaf=dict(recreate=CI, min_ruin_count=2, max_ruin_count=4), search=(HC, BEST), order=RANDOM,
                             steps=10, seed=14),
    "assignment_lists": dict(model="assignment", args=dict(lists=True), leaf=dict(recreate=CI, min_ruin_count=2, max_ruin_count=4, value_candidate_limit=100),
                             search=(LA, COUNT), order=SHUFFLED, steps=10, seed=15),
    "balance_fair": dict(model="balance", args=dict(cap=-2), leaf=dict(recreate=CI), search=(LA, COUNT), order=RANDOM, steps=10, seed=16),
    "balance_counts": dict(model="balance", args=dict(cap=-3), leaf=dict(recreate=FF), search=(HC, BEST), order=RANDOM, steps=10, seed=17),
    "shift": dict(model="shift", args=dict(), leaf=dict(recreate=CI), search=(LA, COUNT), order=RANDOM, steps=10, seed=18),
}
LEVELS = 2
ASSIGNMENT_N, ASSIGNMENT_VALUES = 24, 130
BEST_ORDINALS = (0, 63, 64, 65, 129)  # where the cheapest value of entity e sits (e % 5); entity 5 has it twice, at 10 and 70


def graph(n, e, k, seed, assigned_every=0, all_assigned=False):
    from solverforge_amd import datasets

    g = datasets.make_graph(n, e, k, seed=seed)
    r = datasets.stream(seed + 99, n)
    g["colors"] = (r % np.uint64(k + 1)).astype(np.int64) - 1
    if all_assigned:
        g["colors"] = (r % np.uint64(k)).astype(np.int64)
    if assigned_every:
        keep = np.arange(n) % assigned_every == 0
        g["colors"] = np.where(keep, (r % np.uint64(k)).astype(np.int64), -1)
    return g


def assignment_problem():
    from solverforge_amd import datasets

    n, k = ASSIGNMENT_N, ASSIGNMENT_VALUES
    r = datasets.stream(77, n + n * k)
    values = (r[:n] % np.uint64(k + 1)).astype(np.int64) - 1
    cost = (r[n:] % np.uint64(900)).astype(np.int64).reshape(n, k) + 100
    for e in range(n):
        cost[e, BEST_ORDINALS[e % 5]] = 3 + e
    cost[5, :] = np.maximum(cost[5, :], 50)
    cost[5, 10] = cost[5, 70] = 7  # the best twice: the first wins
    lists = [list(range(k)) for _ in range(n)]
    return values, cost, lists


def problem(name):
    s = SCRIPTS[name]
    a = dict(s["args"])
    if s["model"] == "colouring":
        required, empty_every = a.pop("required", False), a.pop("empty_lists_every", 0)
        g = graph(**a)
        g["required"] = required
        g["value_lists"] = None
        if empty_every:
            g["value_lists"] = [[] if v % empty_every == 1 else list(range(g["n_colors"])) for v in range(g["n"])]
        return g
    if s["model"] == "assignment":
        values, cost, lists = assignment_problem()
        return dict(values=values, cost=cost, value_lists=lists if a["lists"] else None, n=ASSIGNMENT_N, n_values=ASSIGNMENT_VALUES)
    if s["model"] == "balance":
        rng = np.random.default_rng(5)
        bins, sizes = rng.integers(-1, 6, 50).astype(np.int64), rng.integers(1, 9, 50).astype(np.int64)
        return dict(bins=bins, sizes=sizes, n_bins=6, cap=a["cap"], n=50, n_values=6, value_lists=None)
    from test_gpu_runs import _problem

    nurse, day = _problem(5, 8, 3, seed=3)
    return dict(nurse=nurse, day=day, n_nurses=5, n=len(nurse), n_values=5, value_lists=None)


def shape(name):
    """(entities, values, allows_unassigned, value lists) of a script's scalar variable."""
    p = problem(name)
    if SCRIPTS[name]["model"] == "colouring":
        return p["n"], p["n_colors"], not p["required"], p["value_lists"]
    return p["n"], p["n_values"], True, p["value_lists"]


def oracle_model(sfo, name, values=None):
    s, p = SCRIPTS[name], problem(name)
    if s["model"] == "colouring":
        o = sfo.Model.graph_coloring(p["n_colors"], p["adj_off"], p["adj"], p["colors"] if values is None else values)
    elif s["model"] == "assignment":
        o = sfo.Model.assignment(p["values"] if values is None else values, p["cost"], p["n_values"], ex_level=-1)
    elif s["model"] == "balance":
        o = sfo.Model.balance(p["n_bins"], p["bins"] if values is None else values, p["sizes"], w_pair=3, cap=p["cap"])
    else:
        o = sfo.Model.shift_schedule(p["nurse"] if values is None else values, p["day"], p["n_nurses"], limit=2, w_streak=1, count_weight=1)
    o.configure(acceptor=0, forager=2, random_ties=False, selection_order=s["order"], leaves=3, random_seed=s["seed"])
    if p.get("value_lists") is not None:
        o.set_value_lists(p["value_lists"])
    return o


def leaf_of(sfo, name, model, replica=0):
    n, n_values, allows, lists = shape(name)
    return rm.RuinLeaf(sfo, model, n, n_values, SCRIPTS[name]["seed"] + replica, allows_unassigned=allows, value_lists=lists, levels=LEVELS, **SCRIPTS[name]["leaf"])


def search_of(sfo, name, values=None, replica=0, before=(), after=(), search=None, order=None):
    """(oracle model, mirror search) of a script, from its start state or from a replica's working values."""
    s = SCRIPTS[name]
    o = oracle_model(sfo, name, values)
    acceptor, forager = search or s["search"]
    return o, rm.Search(sfo, o, leaf_of(sfo, name, o, replica), s["seed"] + replica, acceptor=acceptor, la_size=LA_SIZE, forager=forager, limit=LIMIT,
                        order=s["order"] if order is None else order, before=before, after=after)


def device_model(name, n_replicas=1, before=(), after=(), leaf=None):
    """The director of a script: the leaves of `before`, the ruin leaf, the leaves of `after`, declared in this order."""
    import solverforge_amd as sfa
    from solverforge_amd.director import ConstraintKind, GpuScoreDirector, SelectorKind

    s, p = SCRIPTS[name], problem(name)
    if s["model"] == "colouring" and (p["required"] or p["value_lists"] is not None):
        d = GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=n_replicas)  # build_graph_coloring's model with a required variable / value lists
        d.add_entity_class(0, p["n"])
        d.add_scalar_variable(0, 0, p["n_colors"], not p["required"], p["colors"])
        d.add_fact_csr(1, p["adj_off"], p["adj"])
        d.add_constraint(ConstraintKind.UNI_UNASSIGNED, 0, level=0, weight=1)
        d.add_constraint(ConstraintKind.CROSS_ADJACENT_EQUAL, 0, fact=1, level=0, weight=1)
    elif s["model"] == "colouring":
        d = sfa.build_graph_coloring(p, n_replicas=n_replicas, leaves=())
    elif s["model"] == "assignment":
        d = sfa.build_assignment(p["values"], p["cost"], p["n_values"], n_replicas=n_replicas, ex_level=-1, leaves=())
    elif s["model"] == "balance":
        d = sfa.build_balance(p["bins"], p["sizes"], p["n_bins"], n_replicas=n_replicas, w_pair=3, cap=p["cap"], leaves=())
    else:
        d = sfa.build_shift_schedule(p["nurse"], p["day"], p["n_nurses"], n_replicas=n_replicas, limit=2, w_streak=1, count_weight=1, leaves=())
    if p.get("value_lists") is not None:
        d.set_value_lists(0, 0, p["value_lists"])
    kinds = {1: SelectorKind.SCALAR_CHANGE, 2: SelectorKind.SCALAR_SWAP}
    for bits in before:
        d.add_selector(kinds[bits], 0)
    d.add_scalar_ruin_selector(0, **(s["leaf"] if leaf is None else leaf))
    for bits in after:
        d.add_selector(kinds[bits], 0)
    return d


def configure(d, name, search=None, order=None, union=None):
    import solverforge_amd as sfa

    s = SCRIPTS[name]
    acceptor, forager = search or s["search"]
    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=LA_SIZE, forager=forager, accepted_count_limit=LIMIT, random_ties=False,
                                 selection_order=s["order"] if order is None else order, random_seed=s["seed"]))
    if union is not None:
        d.configure_union(union)
