"""GPU: the TabuSearch acceptor (tabu_search.rs:64-237) at the three sites that build move signatures on the device (csrc/sf_tabu.h): the
fused scalar engine (scalar change / swap), the wave engine's general replay (nearby list change / swap) and the generic engine (plain and
nearby list change / swap on a list model; scalar and list leaves on a mixed model, which has two scopes).  The oracle cannot run this acceptor, so the tests stand on tests/tabu_mirror.py (pinned on the CPU by
tests/test_tabu_mirror.py) and on what the oracle can still confirm:

1. traced runs, candidate by candidate: every accept flag is the mirror's is_accepted on the signature the mirror builds from an oracle
   model's state BEFORE the step; that model follows by apply_move, which also confirms the traced scores and doability; after every step
   the device's tabu state (best, push counts, tabu tokens, live identities) is the mirror's.  The events that tell the rules apart
   (EVENTS) must all occur over the configurations of the site, judged on the mirror's flags;
2. the same configuration fused -- one launch, two launches, two budgeted launches -- ends in the state the traced run reached;
3. validation: everything that builds no signature is refused at launch with its error code.

Models: a colouring of 70 nodes with 4 colours (past one 64-lane chunk; unassigned allowed, so `to = None` changes occur) and the
36-customer grid CVRP of tests/test_gpu_step_protocol.py (wave and generic sites); a mixed job shop of 12 operations on 3 machines (scalar
class + list class: an operation index and an equal machine index are different tokens); 3 replicas with seeds s + r, 36 steps.  The
traced runs follow replica 0; the policy with all four memories is traced at replicas 1 and 2 as well, at every site, against a mirror
and an oracle model of their own (a wrong arena offset or row stride shows there: fused == traced cannot see it, both kernels share
the address arithmetic).  tests/test_gpu_acceptor_state_at_size.py does the same at launches of several residencies."""
import pytest

import tabu_mirror as tm
from test_gpu_anneal import _graph
from test_gpu_foragers import COUNTERS
from test_gpu_mixed import _jobshop
from test_gpu_step_protocol import LIST_SITES, ORDER_RANDOM, _decide_candidates, _grid_cvrp

pytestmark = pytest.mark.gpu

TABU, LA = 7, 1
R, STEPS, SEED = 3, 36, 5
MIXED_JOBS, MIXED_MACHINES = 4, 3  # 12 operations (scalar class 0: machine_idx) on 3 machines (list class 1: sequence)
# the scope of a site's scalar moves / list moves, and the device packing: scope number, entity token base, value token base (scalar class first)
SCALAR_SCOPE = {"scalar": (0, "color_idx"), "mixed": (0, "machine_idx")}
LIST_SCOPE = {"wave": (0, "visits"), "generic": (0, "visits"), "mixed": (1, "sequence")}
PACKER = {"scalar": tm.ModelPacker({SCALAR_SCOPE["scalar"]: (0, 0, 0)}), "wave": tm.ModelPacker({LIST_SCOPE["wave"]: (0, 0, 0)}),
          "generic": tm.ModelPacker({LIST_SCOPE["generic"]: (0, 0, 0)}),
          "mixed": tm.ModelPacker({SCALAR_SCOPE["mixed"]: (0, 0, 0), LIST_SCOPE["mixed"]: (1, MIXED_JOBS * MIXED_MACHINES, MIXED_MACHINES + 1)})}
# (policy [entity, value, move, undo, aspiration], forager, accepted_count_limit).  AcceptedCount(70): a step spans more than one chunk.
# BestScore reads the whole neighbourhood; FirstAccepted ends the step at the first admissible candidate, so it walks sideways and downhill
# and comes back to what it recorded.  `saturated`: five value tokens (4 colours and None) in a memory of 8 with aspiration off -- once all
# five are held every candidate is tabu and the step applies nothing.  `move` runs the swap leaf alone under BestScore: a swap is its own
# reverse, so the step after any swap meets it again in the move memory.  `undo` under BestScore: the reverse of the change just applied is
# a candidate of the next step and worse than the acceptor's best.
# The list site has four routes: `saturated` there is an entity memory of 8 -- once it holds all four, every move touches a tabu route.
# The generic site runs a plain and a nearby leaf side by side, the other pairing in `all_four` (leaf kinds 4 + 32, 16 + 8).  The mixed model has
# 12 + 3 entity tokens: `saturated` there is an entity memory of 32, which holds all of them before it evicts any.
BOTH = {"scalar": ("change", "swap"), "wave": ("nearby_change", "nearby_swap"), "generic": ("list_change", "nearby_swap"),
        "mixed": ("list_change", "list_swap", "change", "swap")}
ALT = dict(BOTH, generic=("nearby_change", "list_swap"))
SWAP = {"scalar": ("swap",), "wave": ("nearby_swap",), "generic": ("list_swap",), "mixed": ("list_swap", "swap")}
SITE_CONFIGS = {
    "scalar": {
        "entity": ([3, None, None, None, True], 0, 70, BOTH),
        "value": ([None, 2, None, None, True], 1, 0, BOTH),
        "move": ([None, None, 5, None, True], 2, 0, SWAP),
        "undo": ([None, None, None, 5, True], 2, 0, BOTH),
        "all_four": ([4, 2, 6, 6, True], 0, 70, BOTH),
        "best_score": ([2, 1, 3, 3, True], 2, 0, BOTH),
        "saturated": ([None, 8, None, None, False], 2, 0, BOTH),
    },
    "wave": {
        "entity": ([2, None, None, None, True], 0, 70, BOTH),
        "value": ([None, 3, None, None, True], 2, 0, BOTH),
        "move": ([None, None, 5, None, True], 2, 0, SWAP),
        "undo": ([None, None, None, 5, True], 2, 0, BOTH),
        "all_four": ([3, 3, 6, 6, True], 0, 70, BOTH),
        "best_score": ([2, 2, 3, 3, True], 2, 0, BOTH),
        "saturated": ([8, None, None, None, False], 2, 0, BOTH),
    },
    "generic": {
        "entity": ([2, None, None, None, True], 0, 70, BOTH),
        "value": ([None, 3, None, None, True], 2, 0, BOTH),
        "move": ([None, None, 5, None, True], 2, 0, SWAP),
        "undo": ([None, None, None, 5, True], 2, 0, BOTH),
        "all_four": ([3, 3, 6, 6, True], 0, 70, ALT),
        "best_score": ([2, 2, 3, 3, True], 2, 0, BOTH),
        "saturated": ([8, None, None, None, False], 2, 0, BOTH),
    },
    "mixed": {
        "entity": ([3, None, None, None, True], 0, 70, BOTH),
        "value": ([None, 3, None, None, True], 2, 0, BOTH),
        "move": ([None, None, 5, None, True], 2, 0, SWAP),
        "undo": ([None, None, None, 5, True], 2, 0, BOTH),
        "all_four": ([3, 3, 6, 6, True], 0, 70, BOTH),
        "best_score": ([2, 2, 3, 3, True], 2, 0, BOTH),
        "saturated": ([32, None, None, None, False], 2, 0, BOTH),
    },
}
SITES = list(SITE_CONFIGS)
CASES = [(site, name) for site in SITES for name in SITE_CONFIGS[site]]
COMMON_EVENTS = ("refused_by_entity_alone", "refused_by_value_alone", "refused_by_move_alone", "refused_by_undo_alone", "aspirational_accept_of_tabu",
                 "admissible_again_after_eviction", "step_applied_nothing")
EVENTS = {"scalar": COMMON_EVENTS + ("to_none_refused_by_value",), "wave": COMMON_EVENTS + ("intra_list_change_decided",),
          "generic": COMMON_EVENTS + ("intra_list_change_decided",), "mixed": COMMON_EVENTS + ("equal_id_under_the_other_scope_admitted",)}

_memo = {}


class _Events(dict):
    """event -> the first step that showed it; `add` as a set's, so that a run can say how many steps its events needed."""
    step = 0

    def add(self, event):
        self.setdefault(event, self.step)


def _problem():
    return _graph(n=70, e=170, k=4, seed=11)


def _build(site="scalar", n_replicas=R, leaves=None):
    import solverforge_amd as sfa

    leaves = leaves or BOTH[site]
    if site == "scalar":
        return sfa.build_graph_coloring(_problem(), n_replicas=n_replicas, leaves=leaves)
    if site == "mixed":
        return sfa.build_jobshop(_mixed_problem(), n_replicas=n_replicas, bendable=False, leaves=leaves)
    d = sfa.build_cvrp(_grid_cvrp(), n_replicas=n_replicas, leaves=leaves)
    if site == "wave":
        d.set_engine(2)
    return d


def _mixed_problem():
    return _jobshop(n_jobs=MIXED_JOBS, n_machines=MIXED_MACHINES, seed=2)


def _oracle_model(oracle, site, state=None):
    """The oracle Model of a site, from its start state or from a replica's working state (the pair _state returns)."""
    vals, lists = state if state is not None else (None, None)
    if site == "scalar":
        g = _problem()
        return oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"] if vals is None else vals)
    if site == "mixed":
        p = _mixed_problem()
        return oracle.Model.jobshop(p["job"], p["machine_idx"] if vals is None else vals, p["sequences"] if lists is None else lists, bendable=False)
    p = _grid_cvrp()
    return oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"] if lists is None else lists)


def _state(d, site, r):
    """(scalar values or None, lists or None) of a replica."""
    vals = d.working_values(0, 0, replica=r).tolist() if site in SCALAR_SCOPE else None
    lists = [list(x) for x in d.working_lists(1 if site == "mixed" else 0, r)] if site in LIST_SCOPE else None
    return vals, lists


def _oracle_state(o, site):
    vals = o.get_vars(0, 0).tolist() if site in SCALAR_SCOPE else None
    lists = [list(x) for x in o.get_lists(1 if site == "mixed" else 0)] if site in LIST_SCOPE else None
    return vals, lists


def _configure(d, policy, forager, limit, acceptor=TABU, seed=SEED):
    import solverforge_amd as sfa

    d.configure_tabu(*policy)  # before the kind is named: sf_solver_configure takes kind 7 only once its policy was set
    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=5, forager=forager, accepted_count_limit=limit, random_ties=True,
                                 selection_order=ORDER_RANDOM, random_seed=seed))
    d.calculate_score()
    d.phase_start()


def _tabu_tuple(d, r):
    st = d.tabu_state(r)
    best = tuple(st["best"].tolist())
    return (best + (0,) * (4 - len(best)), tuple(st["pushes"]), st["entity"], st["value"], st["moves"], st["undo"])


def _snapshot(d, site, replicas=range(R)):
    """Per replica: (score, best score, working state, the seven counters, tabu state)."""
    scores, best = d.calculate_score(), d.best_scores()
    out = []
    for r in replicas:
        st = d.stats(r)
        out.append((scores[r].tolist(), best[r].tolist(), _state(d, site, r), [st[k] for k in COUNTERS], _tabu_tuple(d, r)))
    assert (d.fresh_score() == scores).all()
    return out


def _signature(site, move, state):
    """The mirror's signature of a traced move, from the working state before the move (values / lists of the oracle model)."""
    a, b, kind = int(move["a"]), int(move["b"]), int(move["kind"])
    vals, lists = state
    if kind <= 1:
        v = lambda x: None if x < 0 else int(x)  # noqa: E731
        if kind == 0:
            return tm.change_signature(SCALAR_SCOPE[site], a, v(vals[a]), v(move["value"]))
        return tm.swap_signature(SCALAR_SCOPE[site], a, b, v(vals[a]), v(vals[b]))
    i, j = int(move["a_pos"]), int(move["b_pos"])
    if kind == 2:  # b_pos is the destination before the removal; the mirror adjusts it
        return tm.list_change_signature(LIST_SCOPE[site], a, i, b, j, int(lists[a][i]))
    assert kind == 3
    return tm.list_swap_signature(LIST_SCOPE[site], a, i, int(lists[a][i]), b, j, int(lists[b][j]))


def trace_replica(oracle, d, site, policy, replica, steps, o=None, packer=None):
    """One replica of a context at the start of a phase under TabuSearch, step by step through sf_solve_step_traced (the launch moves
    every replica one step).  o: the oracle model of that replica's working state (default: the site's start state); it follows the
    replica by apply_move, its own search plays no part.  The mirror starts fresh, as the phase does.  packer: the device packing of
    a model of the site's shape and another size (default: the site's); the scores have the director's level count.  Returns {event:
    the first step that showed it}."""
    if o is None:
        o = _oracle_model(oracle, site)
    packer, L = packer or PACKER[site], d.levels
    mirror = tm.TabuSearch(policy)
    cur = tuple(int(x) for x in o.score()[:L])
    assert tuple(d.calculate_score()[replica].tolist()) == cur
    assert _state(d, site, replica) == _oracle_state(o, site)
    mirror.phase_started(cur)
    events, refused_ids = _Events(), set()
    for step in range(steps):
        events.step = step
        assert _tabu_tuple(d, replica) == tm.packed_state(mirror, packer), (replica, step)
        vals = _oracle_state(o, site)
        gm, gs, gf, gap, gmv = d.solve_step_traced(replica=replica, cap=1 << 15)
        os_, od = o.evaluate_moves(gm)
        doable = (gf & 1) != 0
        assert (doable == (od != 0)).all(), step
        assert (gs[doable] == os_[doable][:, :L]).all(), step
        for mv, sc_row, fl in zip(gm, gs, gf):
            if not fl & 1:
                assert not fl & 2, step  # a candidate that is not doable never reaches the acceptor
                continue
            sc, sig = tuple(int(x) for x in sc_row), _signature(site, mv, vals)
            want = mirror.is_accepted(cur, sc, sig)
            assert bool(fl & 2) == want, (step, mv, sc, sig, mirror.state())
            reasons, asp = mirror.tabu_reasons(sig), mirror.is_aspirational(sc)
            if not want:
                refused_ids.add(sig.move_id)
                for memory in reasons:  # (not in EVENTS: tests/test_gpu_precedence_policies.py asks for these of policies with several memories)
                    events.add("refused_with_%s" % memory)
                if len(reasons) == 1:
                    events.add("refused_by_%s_alone" % next(iter(reasons)))
                if site == "scalar" and "value" in reasons and int(mv["kind"]) == 0 and int(mv["value"]) < 0:
                    events.add("to_none_refused_by_value")
            elif reasons:
                assert asp
                events.add("aspirational_accept_of_tabu")
            elif not asp and sig.move_id in refused_ids:
                events.add("admissible_again_after_eviction")
            if site == "mixed" and want and not reasons and not asp:  # its entity index is tabu under the other scope only
                held = {t for t in mirror.mem["entity"].entries}
                if any((other, e) in held for scope_, e in sig.entity_tokens for other in (SCALAR_SCOPE[site], LIST_SCOPE[site]) if other != scope_):
                    events.add("equal_id_under_the_other_scope_admitted")
            if site in ("wave", "generic") and int(mv["kind"]) == 2 and int(mv["a"]) == int(mv["b"]) and int(mv["b_pos"]) > int(mv["a_pos"]) and (reasons or asp):
                events.add("intra_list_change_decided")  # a forward intra-list change (adjusted destination, one entity token) under a live rule
        applied_sig = None
        if gap:
            applied_sig = _signature(site, gmv, vals)  # from the state before the move
            o.apply_move(gmv)
            assert ((gf & 4) != 0).sum() == 1
        else:
            events.add("step_applied_nothing")
            assert not (gf & 2).any()
        cur = tuple(int(x) for x in o.score()[:L])
        assert tuple(d.calculate_score()[replica].tolist()) == cur, (replica, step)
        mirror.step_ended(cur, applied_sig)
    assert _tabu_tuple(d, replica) == tm.packed_state(mirror, packer), replica
    assert _state(d, site, replica) == _oracle_state(o, site), replica
    return events


def traced_run(oracle, site, policy, forager, limit, leaves, replica=0, n_replicas=R, seed=SEED, steps=STEPS, snapshot_of=None):
    """Replica `replica` of a fresh context of n_replicas (replica r runs seed + r) through trace_replica.  Returns (events seen, the
    snapshot of the replicas snapshot_of -- default: all of them -- after the run)."""
    d = _build(site, n_replicas=n_replicas, leaves=leaves[site])
    _configure(d, policy, forager, limit, seed=seed)
    events = trace_replica(oracle, d, site, policy, replica, steps)
    snap = _snapshot(d, site, range(n_replicas) if snapshot_of is None else snapshot_of)
    d.close()
    return set(events), snap


def _traced(oracle, site, name, replica=0):
    if (site, name, replica) not in _memo:
        _memo[(site, name, replica)] = traced_run(oracle, site, *SITE_CONFIGS[site][name], replica=replica)
    return _memo[(site, name, replica)]


@pytest.mark.parametrize("site,name", CASES)
def test_traced_replay_matches_the_mirror(oracle, site, name):
    events, snap = _traced(oracle, site, name)
    policy = SITE_CONFIGS[site][name][0]
    alone = [k for k, t in zip(tm.MEMORIES, policy[:4]) if t is not None]
    if len(alone) == 1 and name != "saturated":  # a policy with one memory: that memory refuses, alone
        assert "refused_by_%s_alone" % alone[0] in events, sorted(events)
    if name == "saturated":
        assert "step_applied_nothing" in events, sorted(events)
    assert len({str(s[2]) for s in snap}) == R  # replicas with seeds s + r differ from one another


@pytest.mark.parametrize("replica", [1, 2])
@pytest.mark.parametrize("site", SITES)
def test_traced_replay_of_replicas_1_and_2(oracle, site, replica):
    """The fused and the traced kernel reach a replica's tabu row and arena by the same arithmetic, so fused == traced says nothing about
    a wrong stride or a stamp table that spills into the next replica's ring.  Here the mirror and the oracle model follow replica 1
    and replica 2 of the policy with all four memories; the launch moves every replica whichever one is traced, so the run ends in
    the snapshot of the run that traced replica 0."""
    _, snap = _traced(oracle, site, "all_four", replica)
    assert snap == _traced(oracle, site, "all_four")[1]


@pytest.mark.parametrize("site", SITES)
def test_every_event_occurs_at_the_site(oracle, site):
    seen = set().union(*(_traced(oracle, site, name)[0] for name in SITE_CONFIGS[site]))
    assert not [e for e in EVENTS[site] if e not in seen], sorted(seen)


@pytest.mark.parametrize("site,name", CASES)
def test_fused_ends_where_the_traced_run_did(oracle, site, name):
    want = _traced(oracle, site, name)[1]
    for mode in ("one_launch", "two_launches", "two_budgeted_launches"):
        d = _build(site, leaves=SITE_CONFIGS[site][name][3][site])
        _configure(d, *SITE_CONFIGS[site][name][:3])
        if mode == "one_launch":
            d.solve_steps(STEPS)
        else:
            for n in (STEPS // 2, STEPS - STEPS // 2):
                if mode == "two_budgeted_launches":
                    d.solve_moves(n, 1 << 30)  # no replica reaches the budget: every one runs n steps
                else:
                    d.solve_steps(n)
        assert _snapshot(d, site) == want, mode


def test_default_policy_is_move_only_10(oracle):
    import solverforge_amd as sfa

    d = _build(n_replicas=1)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*acceptor kind 7.*sf_solver_configure_tabu"):
        d.configure(sfa.SolverConfig(acceptor=TABU, forager=1, random_seed=SEED))  # the kind is taken only once its policy was set
    d.configure_tabu()  # no argument: the default policy
    d.configure(sfa.SolverConfig(acceptor=TABU, forager=1, random_seed=SEED))
    initial = d.calculate_score()[0].tolist()
    d.phase_start()
    st = d.tabu_state(0)
    assert st["best"].tolist() == initial and st["pushes"] == [0, 0, 0, 0] and not (st["entity"] or st["value"] or st["moves"] or st["undo"])
    d.solve_steps(12)
    st = d.tabu_state(0)
    assert st["pushes"] == [0, 0, 12, 0] and len(st["moves"]) == 10 and not st["undo"]
    d.configure_tabu(None, None, None, None, aspiration_enabled=False)  # all four absent, explicitly
    d.phase_start()
    d.solve_steps(3)
    assert d.tabu_state(0)["pushes"] == [0, 0, 3, 0]


def test_validation(oracle):
    import solverforge_amd as sfa

    # a change of acceptor needs a new phase start: a launch under TabuSearch in a phase started under another acceptor is refused
    d = _build()
    _configure(d, [2, None, None, None, True], 1, 0, acceptor=LA)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.tabu_state(0)
    d.configure(sfa.SolverConfig(acceptor=TABU, late_acceptance_size=5, forager=1, random_seed=SEED))
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*sf_phase_start"):
        d.solve_steps(2)
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*sf_phase_start"):
        d.solve_step_traced(replica=0)
    d.phase_start()
    d.solve_steps(2)
    assert d.tabu_state(2)["pushes"][0] <= 4
    # the provider step prices compound candidates
    g = _problem()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
        d.step_decide_cursor(_decide_candidates(g, 0), replica=0)
    # move tenures above 64; an explicit 0 (the reference's message)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*64"):
        d.configure_tabu(move_tabu_size=65)
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*tabu_search field `value_tabu_size` must be greater than 0"):
        d.configure_tabu(value_tabu_size=0)
    assert g["n"] == 70
    # list models: the block engine (forced) builds no signatures; the reverse leaf's signature has no fixed size; elite migration lists the acceptors it takes
    for site, (engine, leaves, order) in LIST_SITES.items():
        dl = sfa.build_cvrp(_grid_cvrp(), n_replicas=2, leaves=leaves)
        if engine:
            dl.set_engine(engine)
        dl.configure_tabu()
        dl.configure(sfa.SolverConfig(acceptor=TABU, forager=1, selection_order=order, random_seed=SEED))
        dl.calculate_score()
        dl.phase_start()
        if site == "wave":
            dl.solve_steps(2)
            assert dl.wave_layout()[0] == 0  # the general replay, never a FAST kernel
        else:
            with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*tabu search.*" + ("block engine" if site == "block" else "variable-length")):
                dl.solve_steps(2)
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
            dl.migrate_local(1, 1)
    # every other leaf with a variable-length or composite signature
    for leaf in ("sublist_change", "sublist_swap", "kopt"):
        dl = sfa.build_cvrp(_grid_cvrp(), n_replicas=2, leaves=("nearby_change", leaf))
        dl.configure_tabu()
        dl.configure(sfa.SolverConfig(acceptor=TABU, forager=1, random_seed=SEED))
        dl.calculate_score()
        dl.phase_start()
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*tabu search.*variable-length"):
            dl.solve_steps(2)
