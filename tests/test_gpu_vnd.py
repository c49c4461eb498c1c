"""GPU: the Variable Neighborhood Descent phase (vnd/phase.rs:31-404) in the generic engine, at its three kinds of site: list models
(the 36-customer grid CVRP under three neighbourhood orders, one of them with the nearby leaves), a scalar model (a 70-node colouring) and
a mixed model (a job shop with two list neighbourhoods before the scalar one); one more CVRP order puts the permute and 3-opt leaves
first.  The oracle cannot run the phase, so the tests stand on tests/vnd_mirror.py (pinned on the CPU by tests/test_vnd_mirror.py) over
oracle models:

1. traced runs: a short fused LateAcceptance search with seeds s + r takes the 3 replicas apart; then, for every replica and every step
   until it is done, the pulled moves and their order, the scores, the accept bit (strictly better than the current score), the pick, the
   step score and vnd_state are the mirror's;
2. fused runs -- one launch of more steps than any replica needs, two launches, two budgeted launches, solve_vnd -- end where the traced
   runs did: working state, scores, best scores, the seven counters (the step count is the step index), vnd_state; a further launch
   changes nothing; the final state is a local optimum of every neighbourhood by the oracle;
3. the way back to acceptor-forager search, and every refusal with its message;
4. two scripts at a launch of several residencies: the done count after launches that end some descents and not all, and a sample of
   replicas (both sides of every residency boundary, the last ones) against mirrors run to done."""
import numpy as np
import pytest

import vnd_cases as vc
import vnd_mirror as vm
from test_gpu_large_launch import _launch_size, _rows_differ, _sample
from test_gpu_step_protocol import _decide_candidates

pytestmark = pytest.mark.gpu

R, DIVERGE_STEPS, MANY = 3, 5, 200
LA, ORDER_RANDOM = 1, 3
# the seed of the diverging search, picked on the oracle and the mirror so that the three replicas finish their descent at different steps
SEEDS = {"cvrp_reverse_first": 3, "cvrp_swap_first": 3, "cvrp_nearby": 3, "colouring": 3, "jobshop": 31, "cvrp_permute_kopt": 3}
NAMES = list(vc.ALL_SCRIPTS)
_memo = {}


def _t(moves):
    return np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1)


def _la_config(seed):
    import solverforge_amd as sfa

    return sfa.SolverConfig(acceptor=LA, late_acceptance_size=5, forager=0, accepted_count_limit=8, random_ties=True, selection_order=ORDER_RANDOM,
                            random_seed=seed)


def _start(name, n_replicas=R):
    """The director of a script after the diverging search, at the start of a phase under VND."""
    d = vc.device_model(name, n_replicas)
    d.configure(_la_config(SEEDS[name]))
    d.calculate_score()
    d.phase_start()
    d.solve_steps(DIVERGE_STEPS)
    d.configure_vnd()
    d.phase_start()
    return d


def _mirror(oracle, d, name, r):
    values, lists = vc.device_state(d, name, r)
    o = vc.oracle_model(oracle, name, values, lists)
    seed = SEEDS[name] + r
    return o, vm.VndPhase(o, vc.leaf_bits(name), lambda s: oracle.lib().sfo_step_seed(seed, s))


def _snapshot(d, name, r):
    """(score, best score, working state, the seven counters, vnd_state) of a replica."""
    st = d.stats(r)
    return (d.calculate_score()[r].tolist(), d.best_scores()[r].tolist(), vc.device_state(d, name, r), [st[k] for k in vm.COUNTERS], d.vnd_state(r))


def _traced(oracle, name):
    """Every replica step by step through sf_solve_step_traced (the launch moves every replica one step; the run that traces replica r
    answers for replica r).  Returns (snapshots per replica, steps per replica, records per replica)."""
    if name in _memo:
        return _memo[name]
    snaps, steps, records = [], [], []
    for r in range(R):
        d = _start(name)
        o, mirror = _mirror(oracle, d, name, r)
        assert tuple(d.calculate_score()[r].tolist()) == mirror.current
        recs = []
        while not mirror.done:
            assert d.vnd_state(r) == mirror.state(), (r, len(recs))
            cur = mirror.current
            gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 13)
            rec = mirror.step()
            where = (name, r, rec["step_index"])
            assert len(gm) == rec["cursor"] and (_t(gm) == _t(rec["moves"])).all(), where  # the live leaf's pulls in order
            doable = (gf & 1) != 0
            assert doable.tolist() == rec["doable"], where
            assert ((gf >> 8) == rec["k"]).all(), where  # the flags carry the leaf
            want_accept = [ok and vm.accepts(sc, cur) for sc, ok in zip(rec["scores"], rec["doable"])]
            assert [tuple(row) for row, ok in zip(gs.tolist(), rec["doable"]) if ok] == [sc for sc, ok in zip(rec["scores"], rec["doable"]) if ok], where
            assert ((gf & 2) != 0).tolist() == want_accept, where
            picked = np.flatnonzero(gf & 4).tolist()
            assert picked == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), where
            if gap:
                assert tuple(gmv) == tuple(rec["moves"][rec["pick"]]), where
            assert tuple(d.calculate_score()[r].tolist()) == rec["score"], where
            recs.append(rec)
        assert d.vnd_state(r) == mirror.state() and mirror.done
        snap = _snapshot(d, name, r)
        assert snap[0] == list(mirror.current) and snap[1] == list(mirror.best_score) and snap[2] == vc.state_of(o, name)
        assert snap[3] == [mirror.stats[k] for k in vm.COUNTERS], (snap[3], mirror.stats)
        gm, _, _, gap, _ = d.solve_step_traced(replica=r, cap=1 << 13)  # a replica that is done returns nothing and stays as it is
        assert len(gm) == 0 and not gap and _snapshot(d, name, r) == snap
        snaps.append(snap)
        steps.append(len(recs))
        records.append(recs)
    _memo[name] = (snaps, steps, records)
    return _memo[name]


@pytest.mark.parametrize("name", NAMES)
def test_traced_run_matches_the_mirror(oracle, name):
    snaps, steps, records = _traced(oracle, name)
    assert len(set(steps)) == R, steps  # the replicas finish at different steps
    assert all(s[4]["done"] and s[4]["k"] == s[4]["n"] == len(vc.ALL_SCRIPTS[name][1]) for s in snaps)
    everything = [rec for recs in records for rec in recs]
    assert any(rec["cursor"] > 64 for rec in everything) or name == "jobshop"  # more than one chunk (the job shop's cursors hold 56 at most)
    assert any(rec["pick"] is None for rec in everything) and any(rec["pick"] is not None for rec in everything)


def test_the_device_runs_meet_the_edges_of_the_rule(oracle):
    everything = [rec for name in NAMES for recs in _traced(oracle, name)[2] for rec in recs]
    assert any(rec["pick"] is not None and rec["k"] >= 2 for rec in everything)
    assert any(rec["ties"] >= 2 and rec["last_tie"] != rec["pick"] for rec in everything)
    assert any(rec["pick"] is None and rec["not_doable"] > 0 for rec in everything)
    assert any(rec["cursor"] > 64 and rec["cursor"] % 64 for rec in everything)


@pytest.mark.parametrize("name", NAMES)
def test_fused_ends_where_the_traced_run_did(oracle, name):
    want = _traced(oracle, name)[0]
    for mode in ("one_launch", "two_launches", "two_budgeted_launches"):
        d = _start(name)
        if mode == "one_launch":
            d.solve_steps(MANY)
        elif mode == "two_launches":
            d.solve_steps(7)
            d.solve_steps(MANY)
        else:
            d.solve_moves(MANY, 100 if name == "jobshop" else 2000)  # every replica stops this launch at the step that takes it past the budget
            assert not all(d.vnd_state(r)["done"] for r in range(R))
            d.solve_moves(MANY, 1 << 30)
        got = [_snapshot(d, name, r) for r in range(R)]
        assert got == want, mode
        assert (d.fresh_score() == d.calculate_score()).all()
        d.solve_steps(5)  # all are done: nothing changes, not a counter
        assert [_snapshot(d, name, r) for r in range(R)] == want, mode


@pytest.mark.parametrize("name", NAMES)
def test_solve_vnd_ends_in_a_local_optimum(oracle, name):
    want = _traced(oracle, name)[0]
    d = _start(name)
    assert d.vnd_done_count() == 0
    assert d.solve_vnd(3, steps_per_launch=2) < R  # the step limit: 3 steps per replica end no descent here
    assert d.solve_vnd(500, steps_per_launch=16) == R and d.vnd_done_count() == R
    assert [_snapshot(d, name, r) for r in range(R)] == want
    for r in range(R):
        values, lists = vc.device_state(d, name, r)
        assert vm.is_local_optimum(vc.oracle_model(oracle, name, values, lists), vc.leaf_bits(name))


# steps of the second solve_vnd call of test_vnd_at_size: with the 3 before them they end some descents and not all (on the oracle, the
# sampled replicas of a 256-CU launch need 20 to 29 steps on the colouring and 28 to 39 on the CVRP)
AT_SIZE_PARTIAL = {"colouring": 22, "cvrp_nearby": 30}
AT_SIZE_SAMPLE = 16


@pytest.mark.parametrize("name", list(AT_SIZE_PARTIAL))
def test_vnd_at_size(oracle, name):
    """The phase over several residencies (R = 2 * 32 * CUs + 37, the sample of tests/test_gpu_large_launch.py): sf_vnd_done_count reads
    one word of each of R state rows, solve_vnd's launch loop ends on it, and a done replica leaves the step loop while its neighbours
    in the wavefront's workgroup go on.  Every sampled replica is the stand-alone mirror run to done from the device state the
    diverging search left, under the step seeds of random_seed + r."""
    n_rep, u = _launch_size(False)
    sample = _sample(n_rep, u, AT_SIZE_SAMPLE)
    d = _start(name, n_rep)
    mirrors = {r: _mirror(oracle, d, name, r) for r in sample}
    scores = d.calculate_score()
    assert all(tuple(scores[r].tolist()) == mirrors[r][1].current for r in sample)
    assert d.vnd_done_count() == 0

    def done_flags():
        return sum(d.vnd_state(r)["done"] for r in range(n_rep))

    c = d.solve_vnd(3, steps_per_launch=2)  # the step limit: 3 steps per replica end no descent here
    assert c < n_rep and c == d.vnd_done_count() == done_flags(), c
    c = d.solve_vnd(AT_SIZE_PARTIAL[name], steps_per_launch=8)  # some are done, the others still descend
    assert 0 < c < n_rep and c == d.vnd_done_count() == done_flags(), c
    assert d.solve_vnd(500, steps_per_launch=16) == n_rep and d.vnd_done_count() == n_rep == done_flags()
    scores, best = d.calculate_score().copy(), d.best_scores().copy()
    fresh = d.fresh_score()
    assert (fresh == scores).all(), _rows_differ(fresh, scores)
    snaps, steps = {}, []
    for r in sample:
        o, mirror = mirrors[r]
        n = 0
        while not mirror.done:
            mirror.step()
            n += 1
        steps.append(n)
        snap = snaps[r] = _snapshot(d, name, r)
        assert snap[0] == list(mirror.current) and snap[1] == list(mirror.best_score) and snap[2] == vc.state_of(o, name), r
        assert snap[3] == [mirror.stats[k] for k in vm.COUNTERS], (r, snap[3], mirror.stats)
        assert snap[4] == mirror.state() and snap[4]["done"], (r, snap[4])
        assert vm.is_local_optimum(vc.oracle_model(oracle, name, *snap[2]), vc.leaf_bits(name)), r
    print(f"{name}: R={n_rep} sample={len(sample)} mirror steps {sorted(steps)}")
    assert len(set(steps)) >= 3, steps  # the sampled descents end at different steps
    d.solve_steps(5)  # all are done: nothing changes, not a counter
    assert all(_snapshot(d, name, r) == snaps[r] for r in sample)
    assert (d.calculate_score() == scores).all() and (d.best_scores() == best).all()
    d.close()


@pytest.mark.parametrize("name", ["cvrp_swap_first", "colouring"])
def test_return_to_acceptor_forager_search(oracle, name):
    d = _start(name)
    assert d.solve_vnd(500) == R
    seed = 17
    d.configure(_la_config(seed))
    d.phase_start()
    values, lists = vc.device_state(d, name, 0)
    o = vc.oracle_model(oracle, name, values, lists)
    o.configure(acceptor=LA, la_size=5, forager=0, limit=8, random_ties=True, selection_order=ORDER_RANDOM, leaves=sum(vc.leaf_bits(name)),
                max_nearby=vc.ALL_SCRIPTS[name][2], random_seed=seed)
    o.set_sublist_sizes(*vc.SUBLIST_SIZES)
    o.phase_start()
    gm, gs, gf, gap, gmv = d.solve_step_traced(replica=0, cap=1 << 13)
    om, os_, of, oap, omv = o.step_traced()
    assert len(gm) == len(om) > 0 and (_t(gm) == _t(om)).all() and (gf == of).all() and (gs == os_[:, :2]).all()
    assert gap == oap and (not gap or tuple(gmv) == tuple(omv))
    assert vc.device_state(d, name, 0) == vc.state_of(o, name)
    with pytest.raises(Exception, match="INVALID"):
        d.vnd_state(0)  # the phase was not started under VND


def test_validation(oracle):
    import solverforge_amd as sfa

    # kind 8 is no acceptor of the C ABI
    d = vc.device_model("colouring", 2)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*acceptor kind"):
        d.configure(sfa.SolverConfig(acceptor=8, forager=2, random_seed=1))
    # configure_vnd takes effect at the next phase_start
    d.configure(_la_config(1))
    d.calculate_score()
    d.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.vnd_state(0)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.vnd_done_count()
    d.configure_vnd()
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*variable neighborhood descent.*sf_phase_start"):
        d.solve_steps(2)
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*variable neighborhood descent.*sf_phase_start"):
        d.solve_step_traced(replica=0)
    d.phase_start()
    assert d.vnd_state(1) == {"k": 0, "n": 2, "done": False, "idle_steps": 0}
    # the provider step runs an acceptor and a forager
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*sf_step_decide.*variable neighborhood descent"):
        d.step_decide_cursor(_decide_candidates(vc.problem("colouring"), 0), replica=0)
    d.solve_steps(2)
    assert d.stats(0)["step_count"] == 2
    # a forced engine
    for engine, leaves in ((1, ("nearby_change", "nearby_swap")), (2, ("nearby_change", "nearby_swap"))):
        dl = sfa.build_cvrp(vc.problem("cvrp_nearby"), n_replicas=2, leaves=leaves)
        dl.set_engine(engine)
        dl.configure_vnd()
        dl.calculate_score()
        dl.phase_start()
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*variable neighborhood descent.*generic engine only"):
            dl.solve_steps(2)
        with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*elite migration.*variable neighborhood descent"):
            dl.migrate_local(1, 1)
    # the ruin leaf
    dl = sfa.build_cvrp(vc.problem("cvrp_nearby"), n_replicas=2, leaves=("list_change", "ruin"))
    dl.configure_vnd()
    dl.calculate_score()
    dl.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*variable neighborhood descent.*ruin leaf"):
        dl.solve_steps(2)
    # the critical-path precedence leaf
    from solverforge_amd import datasets

    q = datasets.make_precedence_shop(4, 3, seed=2)
    dp = sfa.build_precedence_shop(q, n_replicas=2, leaves=("precedence", "list_change"))
    dp.configure_vnd()
    dp.calculate_score()
    dp.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*variable neighborhood descent.*precedence leaf"):
        dp.solve_steps(2)
    # more leaves than a union holds
    dm = sfa.build_cvrp(vc.problem("cvrp_nearby"), n_replicas=2, leaves=("list_change",) * 13)
    dm.configure_vnd()
    dm.calculate_score()
    dm.phase_start()
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*too many leaves"):
        dm.solve_steps(2)
