"""The model scripts of the Variable Neighborhood Descent tests: a model, its neighbourhoods in order, and how the oracle and the device
build it.  tests/test_vnd_mirror.py runs them on the mirror alone (they must reach the edges of the rule); tests/test_gpu_vnd.py runs
them on the device against the mirror."""
from test_gpu_anneal import _graph
from test_gpu_mixed import _jobshop
from test_gpu_step_protocol import _grid_cvrp

LEAF_BITS = {"change": 1, "swap": 2, "list_change": 4, "list_swap": 8, "nearby_change": 16, "nearby_swap": 32, "list_reverse": 64,
             "sublist_change": 128, "sublist_swap": 256, "kopt": 512, "permute": 8192}
SUBLIST_SIZES, KOPT, PERMUTE = (1, 3), (1, 20), (2, 5)  # sublist sizes; 3-opt (min_segment_len, max_nearby); permute windows
# name -> (model, neighbourhoods in order, max_nearby of the nearby leaves)
SCRIPTS = {
    "cvrp_reverse_first": ("cvrp", ("list_reverse", "list_swap", "list_change", "sublist_change"), 20),
    "cvrp_swap_first": ("cvrp", ("list_swap", "list_reverse", "sublist_swap", "list_change"), 20),
    "cvrp_nearby": ("cvrp", ("nearby_swap", "nearby_change", "list_reverse", "list_change"), 6),
    "colouring": ("colouring", ("change", "swap"), 20),
    "jobshop": ("jobshop", ("list_swap", "list_change", "change"), 20),
}
# on the device only: leaf kinds beyond the nine of the scripts above (list permute, distance-pruned 3-opt) in front of list change
EXTRA_SCRIPTS = {"cvrp_permute_kopt": ("cvrp", ("permute", "kopt", "list_change"), 20)}
ALL_SCRIPTS = dict(SCRIPTS, **EXTRA_SCRIPTS)
LEVELS = 2


def leaf_bits(name):
    return [LEAF_BITS[x] for x in ALL_SCRIPTS[name][1]]


def problem(name):
    model = ALL_SCRIPTS[name][0]
    if model == "cvrp":
        return _grid_cvrp()
    if model == "colouring":
        return _graph(n=70, e=150, k=4, seed=11)
    return _jobshop(n_jobs=4, n_machines=3, seed=2)


def oracle_model(sfo, name, values=None, lists=None):
    """The oracle Model of a script, from its start state or from a replica's working state (values / lists)."""
    model, _, max_nearby = ALL_SCRIPTS[name]
    p = problem(name)
    if model == "cvrp":
        o = sfo.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"] if lists is None else lists)
    elif model == "colouring":
        o = sfo.Model.graph_coloring(p["n_colors"], p["adj_off"], p["adj"], p["colors"] if values is None else values)
    else:
        o = sfo.Model.jobshop(p["job"], p["machine_idx"] if values is None else values, p["sequences"] if lists is None else lists, bendable=False)
    o.configure(acceptor=0, forager=2, random_ties=False, selection_order=0, leaves=sum(leaf_bits(name)), max_nearby=max_nearby)
    o.set_sublist_sizes(*SUBLIST_SIZES)
    if model == "cvrp":
        o.set_kopt(*KOPT)
        o.set_permute(*PERMUTE)
    return o


def device_model(name, n_replicas):
    """The director of a script; its selectors are declared in the order of the neighbourhoods."""
    import solverforge_amd as sfa
    from solverforge_amd.director import SelectorKind

    model, leaves, max_nearby = ALL_SCRIPTS[name]
    p = problem(name)
    if model == "cvrp":
        return sfa.build_cvrp(p, n_replicas=n_replicas, leaves=leaves, max_nearby=max_nearby, sublist_sizes=SUBLIST_SIZES, kopt=KOPT, permute=PERMUTE)
    if model == "colouring":
        assert leaves == ("change", "swap")  # build_graph_coloring declares them in this order
        return sfa.build_graph_coloring(p, n_replicas=n_replicas, leaves=leaves)
    d = sfa.build_jobshop(p, n_replicas=n_replicas, bendable=False, leaves=())  # the model without a selector; then the neighbourhoods in order
    for leaf in leaves:
        kind = {"list_swap": SelectorKind.LIST_SWAP, "list_change": SelectorKind.LIST_CHANGE, "change": SelectorKind.SCALAR_CHANGE,
                "swap": SelectorKind.SCALAR_SWAP}[leaf]
        d.add_selector(kind, 0 if leaf in ("change", "swap") else 1)
    return d


def state_of(sfo_model, name):
    model = ALL_SCRIPTS[name][0]
    values = sfo_model.get_vars(0, 0).tolist() if model != "cvrp" else None
    lists = [list(x) for x in sfo_model.get_lists(1 if model == "jobshop" else 0)] if model != "colouring" else None
    return values, lists


def device_state(d, name, r):
    model = ALL_SCRIPTS[name][0]
    values = d.working_values(0, 0, replica=r).tolist() if model != "cvrp" else None
    lists = [list(x) for x in d.working_lists(1 if model == "jobshop" else 0, r)] if model != "colouring" else None
    return values, lists
