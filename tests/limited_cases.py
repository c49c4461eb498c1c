"""The scripts of the LimitedNeighborhood tests: a model, its leaves in child order, the union order and the limits -- and, for Variable
Neighborhood Descent, the neighbourhoods as groups of those leaves.  tests/test_limited_mirror.py runs them on the mirror alone (they must
reach the edges of the rule); tests/test_gpu_limited.py runs them on the device against the mirror.

The leaves of a search script stand in the default policy's declaration order (list change, list swap, sublist change, list reverse;
scalar change, scalar swap), which is also the oracle's child order, so that a script means the same union whether or not its root union
is a configured one."""
import limited_mirror as lm
import vnd_cases as vc
from test_gpu_mixed import _jobshop

LEAF_BITS, SUBLIST_SIZES, LEVELS = vc.LEAF_BITS, vc.SUBLIST_SIZES, 2
MODEL_LEAVES = {
    "cvrp": ("list_change", "list_swap", "list_reverse"),
    "colouring": ("change", "swap"),
    "jobshop": ("list_change", "list_swap", "change", "swap"),
}
SEQ, RR, ROT, RND, STRAT = lm.ORDERS


def _s(model, order, child=None, root=None, weights=None):
    return {"model": model, "leaves": MODEL_LEAVES[model], "order": order, "child": dict(child or {}), "root": root, "weights": weights}


# name -> script.  child: {leaf index: limit}
SEARCH = {
    # child limits around one 64-lane batch and two, on children longer than 130 (asserted), under every union order
    "colouring_child_63": _s("colouring", STRAT, {1: 63}),
    "colouring_child_64": _s("colouring", SEQ, {0: 64}),
    "cvrp_child_65": _s("cvrp", RR, {0: 65}),
    "cvrp_child_128": _s("cvrp", ROT, {1: 128}),
    "colouring_child_129": _s("colouring", RND, {1: 129, 0: 140}),
    # 0 and 1; a child cut in the step in which another runs dry by itself (list swap: 23 candidates); a limit above the cursor's length
    "jobshop_zero_one": _s("jobshop", STRAT, {0: 0, 1: 1}),
    "jobshop_cut_and_dry": _s("jobshop", STRAT, {0: 30, 2: 40}),
    "jobshop_cut_weighted": _s("jobshop", STRAT, {3: 17}, weights=(2, 1, 0, 3)),
    "jobshop_identity": _s("jobshop", RR, {0: 1000, 3: 59}),
    "colouring_all_zero": _s("colouring", STRAT, {0: 0, 1: 0}),
    # the root limit
    "jobshop_root_1": _s("jobshop", STRAT, root=1),
    "cvrp_root_63": _s("cvrp", STRAT, root=63),
    "colouring_root_64": _s("colouring", RND, root=64),
    "cvrp_root_65": _s("cvrp", SEQ, root=65),
    "colouring_root_129": _s("colouring", STRAT, root=129),
    # both: the child's binds first (and the root's later), the root's binds first (the child's never)
    "colouring_child_then_root": _s("colouring", STRAT, {1: 10}, root=100),
    "cvrp_root_before_child": _s("cvrp", ROT, {0: 60}, root=64),
}

# Variable Neighborhood Descent: groups = leaf counts over `leaves`; orders / limits per neighbourhood; child = per-leaf limits
VND = {
    # "first a cheap truncated neighbourhood, then the union of the two relocation leaves, then the full 2-opt".  At the start the first
    # improving list swap is candidate 3 of its cursor: a limit of 4 keeps it as the last candidate inside the cut, a limit of 3 leaves it
    # just outside, so that the first step is idle (tests/test_limited_mirror.py asserts both).  steps: the tests run so many steps at most.
    "cvrp_inside": {"model": "cvrp", "leaves": ("list_swap", "list_change", "sublist_change", "list_reverse"), "groups": (1, 2, 1),
                    "orders": (SEQ, SEQ, SEQ), "limits": (4, None, None), "child": {}, "steps": 8},
    "cvrp_outside": {"model": "cvrp", "leaves": ("list_swap", "list_change", "sublist_change", "list_reverse"), "groups": (1, 2, 1),
                     "orders": (SEQ, RR, SEQ), "limits": (3, None, None), "child": {2: 500}, "steps": 8},
    # the same union neighbourhood under two orders: they part at a step whose equal bests lie in both children
    "cvrp_union_sequential": {"model": "cvrp", "leaves": ("list_swap", "list_change", "list_reverse"), "groups": (2, 1),
                              "orders": (SEQ, SEQ), "limits": (None, 100), "child": {}, "steps": 40},
    "cvrp_union_stratified": {"model": "cvrp", "leaves": ("list_swap", "list_change", "list_reverse"), "groups": (2, 1),
                              "orders": (STRAT, SEQ), "limits": (None, 100), "child": {}, "steps": 40},
    # a union of three of four leaves: its offset and stride are drawn over 3, not 4
    "jobshop_three": {"model": "jobshop", "leaves": ("change", "list_swap", "list_change", "swap"), "groups": (1, 3),
                      "orders": (SEQ, STRAT), "limits": (20, None), "child": {3: 25}, "steps": 40},
    "colouring_random": {"model": "colouring", "leaves": ("change", "swap"), "groups": (2,), "orders": (RND,), "limits": (300,), "child": {0: 100}, "steps": 40},
    "jobshop_round_robin": {"model": "jobshop", "leaves": ("list_change", "change", "swap", "list_swap"), "groups": (1, 2, 1),
                            "orders": (SEQ, ROT, RR), "limits": (None, 70, None), "child": {}, "steps": 40},
}


def problem(model):
    if model == "cvrp":
        return vc.problem("cvrp_swap_first")
    if model == "colouring":
        return vc.problem("colouring")
    return _jobshop(n_jobs=4, n_machines=3, seed=2)


def leaf_bits(script):
    return [LEAF_BITS[x] for x in script["leaves"]]


def child_limits(script):
    return [script["child"].get(l) for l in range(len(script["leaves"]))]


def hoods(script):
    """[(leaf indices, union order, limit)] of a VND script."""
    out, first = [], 0
    for g, o, lim in zip(script["groups"], script["orders"], script["limits"]):
        out.append((list(range(first, first + g)), o, lim))
        first += g
    return out


def oracle_model(sfo, script, values=None, lists=None, union_order=None, selection_order=0, weights=None):
    """The oracle Model of a script, from its start state or from a replica's working state; its union = the script's leaves."""
    model, p = script["model"], problem(script["model"])
    if model == "cvrp":
        o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"] if lists is None else lists)
    elif model == "colouring":
        o = sfo.Model.graph_coloring(p["n_colors"], p["adj_off"], p["adj"], p["colors"] if values is None else values)
    else:
        o = sfo.Model.jobshop(p["job"], p["machine_idx"] if values is None else values, p["sequences"] if lists is None else lists, bendable=False)
    o.configure(acceptor=0, forager=2, random_ties=False, selection_order=selection_order, leaves=sum(leaf_bits(script)),
                union_order=-1 if union_order is None else union_order)
    o.set_sublist_sizes(*SUBLIST_SIZES)
    if weights is not None:
        o.set_union_weights(weights)
    return o


def device_model(script, n_replicas):
    """The director of a script: its selectors in the order of the script's leaves, no limit set yet."""
    import solverforge_amd as sfa
    from solverforge_amd.director import SelectorKind

    model, leaves, p = script["model"], script["leaves"], problem(script["model"])
    if model == "cvrp":
        return sfa.build_cvrp(p, n_replicas=n_replicas, leaves=leaves, sublist_sizes=SUBLIST_SIZES)
    if model == "colouring":
        assert leaves == ("change", "swap")
        return sfa.build_graph_coloring(p, n_replicas=n_replicas, leaves=leaves)
    d = sfa.build_jobshop(p, n_replicas=n_replicas, bendable=False, leaves=())
    for leaf in leaves:
        kind = {"list_swap": SelectorKind.LIST_SWAP, "list_change": SelectorKind.LIST_CHANGE, "change": SelectorKind.SCALAR_CHANGE,
                "swap": SelectorKind.SCALAR_SWAP}[leaf]
        d.add_selector(kind, 0 if leaf in ("change", "swap") else 1)
    return d


def apply_limits(d, script):
    """The script's limits on its director (search: union order, weights, leaf and root limits; VND: groups, orders, limits)."""
    for l in range(len(script["leaves"])):
        d.limit_selector(l, script["child"].get(l))
    if "groups" in script:
        d.set_vnd_neighborhoods(list(script["groups"]), script["orders"], script["limits"])
    else:
        d.configure_union(script["order"], script["weights"])
        d.limit_union(script["root"])


HILL_CLIMBING, LATE_ACCEPTANCE, ACCEPTED_COUNT, BEST_SCORE = 0, 1, 0, 2
CONFIGS = ((HILL_CLIMBING, BEST_SCORE), (HILL_CLIMBING, ACCEPTED_COUNT), (LATE_ACCEPTANCE, BEST_SCORE), (LATE_ACCEPTANCE, ACCEPTED_COUNT))
LA_SIZE, ACCEPTED_LIMIT, ORDER_RANDOM, STEPS, SEED = 5, 3, 3, 4, 7


def search_mirror(sfo, script, seed, acceptor, forager, values=None, lists=None):
    """The step mirror of a search script under (acceptor, forager), from the start state or a replica's."""
    o = oracle_model(sfo, script, values, lists)
    return o, lm.LimitedSearch(sfo, o, leaf_bits(script), seed, union_order=script["order"], weights=script["weights"], child_limits=child_limits(script),
                               root_limit=script["root"], acceptor=acceptor, la_size=LA_SIZE, forager=forager, limit=ACCEPTED_LIMIT, order=ORDER_RANDOM)


def vnd_mirror(sfo, script, seed, values=None, lists=None):
    o = oracle_model(sfo, script, values, lists)
    return o, lm.LimitedVnd(sfo, o, leaf_bits(script), hoods(script), lambda s: sfo.lib().sfo_step_seed(seed, s), child_limits(script))


def state_of(sfo_model, script):
    model = script["model"]
    values = sfo_model.get_vars(0, 0).tolist() if model != "cvrp" else None
    lists = [list(x) for x in sfo_model.get_lists(1 if model == "jobshop" else 0)] if model != "colouring" else None
    return values, lists


def device_state(d, script, r):
    model = script["model"]
    values = d.working_values(0, 0, replica=r).tolist() if model != "cvrp" else None
    lists = [list(x) for x in d.working_lists(1 if model == "jobshop" else 0, r)] if model != "colouring" else None
    return values, lists
