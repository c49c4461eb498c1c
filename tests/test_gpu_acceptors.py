"""GPU: the GreatDeluge (great_deluge.rs:89-129) and StepCountingHillClimbing (step_counting.rs:85-129) acceptors in every place that
runs a local-search step: the block engine, the wave engine's general replay, the generic engine, the fused scalar engine and the
host-driven provider step.  The oracle cannot run these acceptors, so the tests stand on what it CAN say and on tests/acceptor_mirror.py
(pinned on the CPU by tests/test_acceptor_mirror.py):

1. exact equivalences with the unchanged oracle: StepCounting(limit 0) is HillClimbing; GreatDeluge(rain_speed 0) is
   LateAcceptance(size > steps) -- both reduce to `sc >= initial`, because the step score never falls below the initial score under either;
2. traced runs, candidate by candidate: every accept flag is the mirror's is_accepted(cur, sc) (of the candidates that reach the acceptor: on
   these models every doable one; trace_replica takes the predicate, tests/test_gpu_precedence_policies.py passes the precedence
   engine's), the acceptor state after every step is the mirror's, an oracle model that follows by apply_move confirms the traced scores and doability.  The events that tell the rules apart
   (EVENTS) must all occur PER SITE, not per run: the water-level events belong to GreatDeluge and the count events to StepCounting, so no
   single run can hold all six; the three runs of a site (TRACE) together must, the GreatDeluge run holding its two and the FirstAccepted
   StepCounting run its two.  These runs follow replica 0; the two FirstAccepted runs are traced at replicas 1 and 2 as well, against a
   mirror and an oracle model of their own (fused == traced cannot see a wrong state-row stride: both kernels share the arithmetic);
   tests/test_gpu_acceptor_state_at_size.py does the same at launches of several residencies;
3. the same configuration fused (two launches; two budgeted launches) ends in the state the traced run reached;
4. validation.

Models: the tying ones of tests/test_gpu_step_protocol.py (36-customer grid CVRP, 60-node colouring), 3 replicas, 40 steps."""
import numpy as np
import pytest

import acceptor_mirror as am
from test_gpu_anneal import _graph
from test_gpu_foragers import COUNTERS
from test_gpu_step_protocol import (GRAPH_N, GRAPH_SEED, LEAF_BITS, LIST_SEED, LIST_SITES, ORDER_RANDOM, _decide_candidates, _decide_graph, _differ,
                                    _grid_cvrp)

pytestmark = pytest.mark.gpu

HC, LA, GD, SC = 0, 1, 5, 6
R, STEPS, DECIDE_STEPS = 3, 40, 12
LA_BIG = 64  # a history longer than the run: every slot still holds the initial score
SITES = list(LIST_SITES) + ["scalar"]
# the equivalences: (new acceptor, its parameter, the oracle's acceptor, forager, accepted_count_limit).  AcceptedCount(70): more than one chunk per step
EQUIV = {"sc0_is_hc": (SC, 0, HC, 2, 0), "gd0_is_la": (GD, 0.0, LA, 0, 70)}
# the traced runs, (acceptor, parameter, forager, accepted_count_limit).  FirstAccepted ends a step at the first accepted candidate: an open
# door walks anywhere (the count reaches the limit, a later climb resets it), rising water is what lets a worse candidate through.  BestScore
# reads the whole neighbourhood: behind a closed door at a local optimum the step applies nothing.  The three runs of a site together must
# contain every event of EVENTS.
TRACE = {"gd_first": (GD, 0.04, 1, 0), "sc_first": (SC, 3, 1, 0), "sc_best": (SC, 3, 2, 0)}
EVENTS = ("accepted_through_water_only", "refused_below_water", "equal_to_cur_refused", "step_applied_nothing", "since_reached_limit", "since_reset_afterwards")

_memo = {}


class _Events(dict):
    """event -> the first step that showed it; `add` as a set's, so that a run can say how many steps its events needed."""
    step = 0

    def add(self, event):
        self.setdefault(event, self.step)


def _build(site, n_replicas=R):
    import solverforge_amd as sfa

    if site == "scalar":
        return sfa.build_graph_coloring(_graph(n=GRAPH_N, e=150, k=4, seed=11), n_replicas=n_replicas)
    engine, leaves, _ = LIST_SITES[site]
    d = sfa.build_cvrp(_grid_cvrp(), n_replicas=n_replicas, leaves=leaves)
    if engine:
        d.set_engine(engine)
    return d


def _oracle_model(oracle, site):
    if site == "scalar":
        g = _graph(n=GRAPH_N, e=150, k=4, seed=11)
        return oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
    p = _grid_cvrp()
    return oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])


def _site_cfg(oracle, site):
    """(selection order, oracle leaf bits, seed) of a site."""
    if site == "scalar":
        return ORDER_RANDOM, oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, GRAPH_SEED
    _, leaves, order = LIST_SITES[site]
    return order, sum(LEAF_BITS[x] for x in leaves), LIST_SEED


def _configure(d, acceptor, param, forager, limit, order, seed, la_size=LA_BIG):
    import solverforge_amd as sfa

    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=la_size, forager=forager, accepted_count_limit=limit, random_ties=True,
                                 selection_order=order, random_seed=seed))
    if acceptor == GD:
        d.configure_great_deluge(param)
    if acceptor == SC:
        d.configure_step_counting(param)
    d.calculate_score()
    d.phase_start()


def _state(d, site, r):
    return d.working_values(0, 0, replica=r).tolist() if site == "scalar" else d.working_lists(0, r)


def _snapshot(d, site, with_acceptor, replicas=range(R)):
    """Per replica: (score, best score, working state, the seven counters, acceptor state)."""
    scores, best = d.calculate_score(), d.best_scores()
    out = []
    for r in replicas:
        st = d.stats(r)
        ax = d.acceptor_state(r) if with_acceptor else None
        out.append((scores[r].tolist(), best[r].tolist(), _state(d, site, r), [st[k] for k in COUNTERS],
                    None if ax is None else (ax[0].tolist(), ax[1].tolist(), ax[2])))
    assert (d.fresh_score() == scores).all()
    return out


def _oracle_run(oracle, site, acceptor, forager, limit):
    """Per replica: (score, best score, state, counters) of the oracle's run of STEPS steps -- computed once per configuration."""
    key = ("oracle", site, acceptor, forager, limit)
    if key not in _memo:
        order, bits, seed = _site_cfg(oracle, site)
        out = []
        for r in range(R):
            o = _oracle_model(oracle, site)
            o.configure(acceptor=acceptor, la_size=LA_BIG, forager=forager, limit=limit, random_ties=True, selection_order=order, leaves=bits, random_seed=seed + r)
            o.phase_start()
            o.steps(STEPS)
            st = o.stats()
            state = o.get_vars(0, 0).tolist() if site == "scalar" else o.get_lists(0)
            out.append((o.score()[:2].tolist(), o.best_score()[:2].tolist(), state, [st[k] for k in COUNTERS]))
        _memo[key] = out
    return _memo[key]


# ---- 1. exact equivalences against the unchanged oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(EQUIV))
@pytest.mark.parametrize("site", SITES)
def test_equivalence_fused(oracle, site, which):
    acceptor, param, o_acceptor, forager, limit = EQUIV[which]
    want = _oracle_run(oracle, site, o_acceptor, forager, limit)
    if which == "gd0_is_la":  # LateAcceptance over the initial score is not HillClimbing here, or the equivalence would show nothing
        assert _differ(want, _oracle_run(oracle, site, HC, forager, limit), 2)
    d = _build(site)
    order, _, seed = _site_cfg(oracle, site)
    _configure(d, acceptor, param, forager, limit, order, seed)
    d.solve_steps(STEPS // 2)
    d.solve_steps(STEPS - STEPS // 2)
    for r, (got, exp) in enumerate(zip(_snapshot(d, site, True), want)):
        assert got[:4] == tuple(exp), (r, got[:2], exp[:2])


def _decide_oracle(oracle, o_acceptor, forager, limit):
    key = ("decide", o_acceptor, forager, limit)
    if key not in _memo:
        g = _decide_graph(oracle)
        out = []
        for r in range(2):
            o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
            o.configure(acceptor=o_acceptor, la_size=LA_BIG, forager=forager, limit=limit, random_ties=True, selection_order=ORDER_RANDOM, leaves=3,
                        random_seed=GRAPH_SEED + r)
            o.phase_start()
            steps = []
            for step in range(DECIDE_STEPS):
                sc, fl, sel = o.step_cursor(_decide_candidates(g, step))
                steps.append((sc[:, :2].copy(), fl.copy(), sel))
            st = o.stats()
            out.append((steps, o.score()[:2].tolist(), o.best_score()[:2].tolist(), o.get_vars(0, 0).tolist(), [st[k] for k in COUNTERS]))
        _memo[key] = out
    return _memo[key]


@pytest.mark.parametrize("which", list(EQUIV))
def test_equivalence_provider_step(oracle, which):
    """sf_step_decide_cursor against Model.step_cursor: the candidates come from the host, one launch per step and replica."""
    import solverforge_amd as sfa

    acceptor, param, o_acceptor, forager, limit = EQUIV[which]
    want = _decide_oracle(oracle, o_acceptor, forager, limit)
    if which == "gd0_is_la":
        assert _differ(want, _decide_oracle(oracle, HC, forager, limit), 3)
    g = _decide_graph(oracle)
    d = sfa.build_graph_coloring(g, n_replicas=2)
    _configure(d, acceptor, param, forager, limit, ORDER_RANDOM, GRAPH_SEED)
    for step in range(DECIDE_STEPS):
        cands = _decide_candidates(g, step)
        for r in range(2):
            gs, gf, gsel = d.step_decide_cursor(cands, replica=r)
            os_, of, osel = want[r][0][step]
            assert len(gf) == len(of) and (gf == of).all(), (step, r)
            assert (gs == os_).all() and gsel == osel, (step, r)
    scores, best = d.calculate_score(), d.best_scores()
    for r, (_, osc, obest, ovals, ost) in enumerate(want):
        st = d.stats(r)
        assert scores[r].tolist() == osc and best[r].tolist() == obest and d.working_values(0, 0, replica=r).tolist() == ovals, r
        assert [st[k] for k in COUNTERS] == ost, r
    assert (d.fresh_score() == scores).all()


# ---- 2. traced replay against the mirror ---------------------------------------------------------------------------------------------
def _acceptor_tuple(d, r):
    level, incr, since = d.acceptor_state(r)
    return tuple(level.tolist()), tuple(incr.tolist()), since


def _doable(record, sc, cur):
    """The default `consult` of trace_replica: every doable candidate reaches the acceptor."""
    return True


def trace_replica(oracle, d, site, acceptor, param, replica, steps, o=None, consult=_doable):
    """One replica of a context at the start of a phase under GreatDeluge / StepCounting, step by step through sf_solve_step_traced (the
    launch moves every replica one step).  The oracle model follows that replica by apply_move from the site's start state: its own
    search code plays no part.  o: the oracle model of the replica's working state (default: the site's start state; any list model on
    class 0 or the site "scalar").  consult(record, sc, cur): does a DOABLE candidate reach the acceptor?  On the models of this file
    every doable candidate does (the default); a move with Move::requires_score_improvement (the critical-path leaf's multi-swap,
    evaluation.rs:95-113) is scored and counted and reaches the acceptor only when it beats the last step score
    (tests/test_gpu_precedence_policies.py passes that predicate).  The accept flag is `doable and consult and mirror.is_accepted`.
    Returns {event: the first step that showed it}; "gate_alone_refused": a doable candidate the acceptor on its own would have accepted
    was kept from it by `consult`."""
    if o is None:
        o = _oracle_model(oracle, site)
    mirror = am.GreatDeluge(param) if acceptor == GD else am.StepCounting(param)
    cur = tuple(int(x) for x in o.score()[:2])
    assert tuple(d.calculate_score()[replica].tolist()) == cur
    mirror.phase_started(cur)
    events, reached = _Events(), False
    for step in range(steps):
        events.step = step
        assert _acceptor_tuple(d, replica) == mirror.state(), (replica, step)
        gm, gs, gf, gap, gmv = d.solve_step_traced(replica=replica, cap=1 << 17)
        os_, od = o.evaluate_moves(gm)
        doable = (gf & 1) != 0
        assert (doable == (od != 0)).all(), step
        assert (gs[doable] == os_[doable][:, :2]).all(), step
        for rec, sc_row, fl in zip(gm, gs, gf):
            sc = tuple(int(x) for x in sc_row)
            if not fl & 1:
                assert not fl & 2, step
                continue
            reaches = bool(consult(rec, sc, cur))
            want = reaches and mirror.is_accepted(cur, sc)
            assert bool(fl & 2) == want, (step, rec, sc, cur, mirror.state())
            if not reaches:
                if mirror.is_accepted(cur, sc):
                    events.add("gate_alone_refused")
                continue
            if acceptor == GD:
                if want and not sc > cur:
                    events.add("accepted_through_water_only")
                if not want:
                    events.add("refused_below_water")
                    assert sc < mirror.water
            if not want and sc == cur:
                events.add("equal_to_cur_refused")
        if gap:
            o.apply_move(gmv)
            assert ((gf & 4) != 0).sum() == 1
        else:
            events.add("step_applied_nothing")
            assert not (gf & 2).any()
        cur = tuple(int(x) for x in o.score()[:2])
        assert tuple(d.calculate_score()[replica].tolist()) == cur, (replica, step)
        mirror.step_ended(cur)
        if acceptor == SC:
            if mirror.since >= mirror.limit:
                events.add("since_reached_limit")
                reached = True
            if reached and mirror.since == 0:
                events.add("since_reset_afterwards")
    assert _acceptor_tuple(d, replica) == mirror.state(), replica
    assert _state(d, site, replica) == (o.get_vars(0, 0).tolist() if site == "scalar" else o.get_lists(0)), replica
    return events


def traced_run(oracle, site, acceptor, param, forager, limit, steps=STEPS, replica=0, n_replicas=R, seed=None, snapshot_of=None):
    """Replica `replica` of a fresh context of n_replicas (replica r runs seed + r; default: the site's seed) through trace_replica.
    Returns (events seen, the snapshot of the replicas snapshot_of -- default: all of them -- after the run)."""
    d = _build(site, n_replicas=n_replicas)
    order, _, site_seed = _site_cfg(oracle, site)
    _configure(d, acceptor, param, forager, limit, order, site_seed if seed is None else seed)
    events = trace_replica(oracle, d, site, acceptor, param, replica, steps)
    snap = _snapshot(d, site, True, range(n_replicas) if snapshot_of is None else snapshot_of)
    d.close()
    return set(events), snap


def _traced(oracle, site, run, replica=0):
    key = ("traced", site, run, replica)
    if key not in _memo:
        _memo[key] = traced_run(oracle, site, *TRACE[run], replica=replica)
    return _memo[key]


@pytest.mark.parametrize("site", SITES)
def test_traced_replay_matches_the_mirror(oracle, site):
    seen = set().union(*(_traced(oracle, site, run)[0] for run in TRACE))
    assert not [e for e in EVENTS if e not in seen], sorted(seen)
    assert {"accepted_through_water_only", "refused_below_water"} <= _traced(oracle, site, "gd_first")[0]
    assert {"since_reached_limit", "since_reset_afterwards"} <= _traced(oracle, site, "sc_first")[0]


@pytest.mark.parametrize("replica", [1, 2])
@pytest.mark.parametrize("run", ["gd_first", "sc_first"])
@pytest.mark.parametrize("site", SITES)
def test_traced_replay_of_replicas_1_and_2(oracle, site, run, replica):
    """The fused and the traced kernel reach a replica's acceptor-state row by the same arithmetic, so fused == traced says nothing about
    a wrong stride or an aliased row.  Here the mirror and the oracle model follow replica 1 and replica 2; the launch moves every
    replica whichever one is traced, so the run ends in the snapshot of the run that traced replica 0."""
    _, snap = _traced(oracle, site, run, replica)
    assert snap == _traced(oracle, site, run)[1]


# ---- 3. fused == traced ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(TRACE))
@pytest.mark.parametrize("site", SITES)
def test_fused_ends_where_the_traced_run_did(oracle, site, run):
    want = _traced(oracle, site, run)[1]
    assert len({str(w[2]) for w in want}) == R  # replicas with seeds s + r differ from one another
    order, _, seed = _site_cfg(oracle, site)
    for budgeted in (False, True):
        d = _build(site)
        _configure(d, *TRACE[run], order, seed)
        for n in (STEPS // 2, STEPS - STEPS // 2):
            if budgeted:
                d.solve_moves(n, 1 << 30)  # the budgeted launch: no replica reaches the budget, every one runs n steps
            else:
                d.solve_steps(n)
        assert _snapshot(d, site, True) == want, budgeted


# ---- 4. validation --------------------------------------------------------------------------------------------------------------------
def test_validation(oracle):
    import solverforge_amd as sfa

    d = _build("wave")
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(sfa.SolverForgeError, match="INVALID"):
            d.configure_great_deluge(bad)
    d.configure_great_deluge(-0.5)  # any finite value is data
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*acceptor kind"):
        d.configure(sfa.SolverConfig(acceptor=7))
    # LateAcceptance + AcceptedCount + SelectionOrder::Random takes this model to a FAST kernel; the new acceptors never do
    _configure(d, LA, None, 0, 70, ORDER_RANDOM, LIST_SEED, la_size=5)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.acceptor_state(0)
    d.solve_steps(2)
    assert d.wave_layout()[0] >= 1
    for acceptor, param in ((GD, 0.001), (SC, 100)):
        _configure(d, acceptor, param, 0, 70, ORDER_RANDOM, LIST_SEED, la_size=5)
        d.solve_steps(2)
        assert d.wave_layout()[0] == 0, acceptor
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
            d.migrate_local(1, 1)
        level, incr, since = d.acceptor_state(1)
        assert len(level) == len(incr) == 2 and since <= 2


def test_defaults_are_the_reference_builder_s(oracle):
    """Without a configure_great_deluge / configure_step_counting call: rain_speed 0.001, step_count_limit 100 (builder/acceptor.rs:242-245,
    215-219)."""
    import solverforge_amd as sfa

    p = _grid_cvrp()
    p["matrix"] = p["matrix"] * 10  # distances large enough for a thousandth of the initial score to be a whole number
    d = sfa.build_cvrp(p, n_replicas=1, leaves=LIST_SITES["generic"][1])
    d.configure(sfa.SolverConfig(acceptor=GD, random_seed=1))
    initial = d.calculate_score()[0].tolist()
    d.phase_start()
    level, incr, since = d.acceptor_state(0)
    assert level.tolist() == initial and incr.tolist() == [am.multiply_level(abs(x), 0.001) for x in initial] and since == 0
    assert any(incr.tolist())
    d.configure(sfa.SolverConfig(acceptor=SC, forager=1, random_seed=1))
    d.phase_start()
    mirror = am.StepCounting(100)
    mirror.phase_started(initial)
    for step in range(4):  # FirstAccepted behind an open door: the first doable candidate, whatever its score
        gm, gs, gf, gap, gmv = d.solve_step_traced(replica=0)
        first = int(np.flatnonzero(gf & 1)[0])
        assert gap and gf[first] & 2 and len(gf) == first + 1, step
        mirror.step_ended(tuple(d.calculate_score()[0].tolist()))
        assert d.acceptor_state(0)[2] == mirror.since, step
