"""GPU tests (through the C ABI) of every fused search engine at launches of several residencies.

The benchmark and every wall-clock solve run tens of thousands of replicas per launch; the other parity tests run 1 to 12.  Here every
engine that runs one wavefront per replica (wave, scalar, generic) is launched with R = 2 * 32 * CUs + 37 replicas of a small model -- 32
is the most wavefronts a CU holds, so whatever occupancy the host plan picks the launch spans more than two residencies, workgroups are
dispatched into LDS and wave slots that earlier ones have left, and the launch ends in a ragged workgroup of a ragged residency.  The
block engine (one 1,024-thread workgroup per replica, at most two per CU) runs R = 2 * 2 * CUs + 5.  The CU count is read from the device.

Replica r is a function of random_seed + r and nothing else (step seeds, the annealing stream and the ruin stream all follow that rule),
so every case checks, after 20 to 60 steps in two launches (SimulatedAnnealing on the scalar engine: 300, so that its calibration
completes; the list engines run SimulatedAnnealing and every site but the block engine DiversifiedLateAcceptance too):

  1. a sample of replicas against the CPU oracle configured with random_seed + r: lists / values, score, best score, counters (and
     temperatures bit for bit under SimulatedAnnealing).  The sample always holds 0, 1, 3, 4, 5, 63, 64, R - 1, R - 2, R - 5 and both sides of
     the first and the second residency boundary (u - 1, u, 2u - 1, 2u with u = 32 * CUs; the block engine's u = 2 * CUs); the rest is a
     fixed-seed draw.  Its size is bounded by the oracle's time (about ten CPU seconds per test at most);
  2. every replica: incremental score == full recalculation, best score >= score;
  3. the step counters of all replicas sum to R * steps (nobody skipped, nobody run twice);
  4. shift invariance over all replicas: a second context seeded random_seed + 5 (odd, no multiple of the workgroup size: every
     trajectory lands in another wave slot, workgroup and residency) gives scores_B[:R - 5] == scores_A[5:], best scores likewise.  This
     compares the library with itself; check 1 anchors it, and together they extend the oracle's verdict from the sample to every index;
  5. on the reference alone: the sampled oracle runs end in pairwise distinct lists / values (a library that ran every replica on one
     seed could not pass on ties).

Each case asserts the kernel path it took (sf_list_wave_layout / sf_list_arith_flags / sf_solver_get_engine).  Two further tests run
sf_solve_moves (replicas stop after different step counts) and sf_portfolio_migrate_local (n_elite 64, n_replace R / 4, the ranking rule
restated in numpy) at the same size."""
import functools
import subprocess
import sys
import time

import numpy as np
import pytest

from test_gpu_arith_edges import COUNTERS, DEFAULT_POLICY, LEAF_BITS, NEARBY, SIX_LEAVES, U16_LAST, U16_OUT, UNREACHABLE, _top_problem

pytestmark = pytest.mark.gpu

MAXN = 10
SEED = 7_000  # replica r of context A runs random_seed SEED + r
SHIFT = 5     # context B: SEED + SHIFT
WAVES_PER_CU = 32  # the most wavefronts a CU holds
BLOCKS_PER_CU = 2  # 1,024-thread workgroups per CU
SA, DLA = 3, 4
GENERIC_THREE = ("nearby_change", "nearby_swap", "list_reverse")  # a third leaf takes a list model to the generic engine


@functools.lru_cache(maxsize=None)
def _cus():
    """The device's CU count as torch reports it, asked once, in a child process: torch bundles a HIP runtime of its own next to the one
    the library links, and a process that has initialised both aborts in their exit-time destructors (bench.py leaves through os._exit
    for that reason; tests/test_portfolio_gloo.py keeps the pytest process torch-free too)."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    cus = int(out.split()[-1])
    assert cus > 0
    return cus


def _launch_size(block):
    """(R, u): the replicas of the launch and the largest possible residency of the engine."""
    u = (BLOCKS_PER_CU if block else WAVES_PER_CU) * _cus()
    return 2 * u + (5 if block else 37), u


def _sample(R, u, n):
    must = {0, 1, 3, 4, 5, 63, 64, R - 1, R - 2, R - 5, u - 1, u, 2 * u - 1, 2 * u}
    assert all(0 <= r < R for r in must), (R, u)
    rest = [int(r) for r in np.random.default_rng(20241).permutation(R) if int(r) not in must]
    return sorted(must) + sorted(rest[:max(0, n - len(must))])


def _lex_ge(a, b):
    """Row by row: a >= b as lexicographic scores."""
    ge = np.ones(len(a), dtype=bool)
    open_ = np.ones(len(a), dtype=bool)
    for k in range(a.shape[1]):
        ge[open_ & (a[:, k] < b[:, k])] = False
        open_ &= a[:, k] == b[:, k]
    return ge


def _rows_differ(a, b):
    return np.flatnonzero((a != b).any(axis=1))[:8]


# ---- the cases: a device context and an oracle of one configuration -----------------------------------------------------------------
def _oracle_acceptor(acceptor):
    """The oracle takes SimulatedAnnealing and DiversifiedLateAcceptance as LateAcceptance plus a configure call of their own."""
    return 1 if acceptor in (SA, DLA) else acceptor


def _configure_acceptor(case, d, seed):
    if case.acceptor == SA:
        d.configure_annealing(mode=2, calibration_sample_size=case.sample_size, seed=seed)
    if case.acceptor == DLA:
        d.configure_diversified(case.tolerance)


def _configure_oracle_acceptor(case, o, seed):
    if case.acceptor == SA:
        o.configure_annealing(mode=2, sample_size=case.sample_size, seed=seed)
    if case.acceptor == DLA:
        o.configure_diversified(case.la, case.tolerance)


class _Cvrp:
    levels = 2

    def __init__(self, problem, leaves, engine=None, acceptor=1, forager=0, la=24, limit=64, ruin=(2, 5, 10), steps=(20, 20), n_sample=48,
                 env=(), path=None, block=False, sample_size=24, tolerance=0.02):
        self.p, self.leaves, self.engine, self.acceptor, self.forager, self.la, self.limit, self.ruin = problem, leaves, engine, acceptor, forager, la, limit, ruin
        self.steps, self.n_sample, self.env, self.path, self.block = steps, n_sample, dict(env), path, block
        self.sample_size, self.tolerance, self.anneal = sample_size, tolerance, acceptor == SA

    def device(self, R, seed):
        import solverforge_amd as sfa

        p = self.p() if callable(self.p) else self.p
        self.p = p
        d = sfa.build_cvrp(p, n_replicas=R, leaves=self.leaves, ruin=self.ruin, max_nearby=MAXN)
        if self.engine is not None:
            d.set_engine(self.engine)
        d.configure(sfa.SolverConfig(acceptor=self.acceptor, late_acceptance_size=self.la, forager=self.forager, accepted_count_limit=self.limit,
                                     random_seed=seed))
        _configure_acceptor(self, d, seed)
        return d

    def cpu(self, oracle, seed):
        p = self.p() if callable(self.p) else self.p
        self.p = p
        o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
        o.configure(acceptor=_oracle_acceptor(self.acceptor), la_size=self.la, forager=self.forager, limit=self.limit, leaves=sum(LEAF_BITS[x] for x in self.leaves),
                    random_seed=seed, max_nearby=MAXN)
        if "ruin" in self.leaves:
            o.set_ruin(self.ruin[0], self.ruin[1], self.ruin[2], variable_name="visits")
        _configure_oracle_acceptor(self, o, seed)
        return o

    def device_state(self, d, r):
        return d.working_lists(0, r)

    def cpu_state(self, o):
        return o.get_lists(0)


class _Graph:
    levels = 2
    block = False
    env = {}

    def __init__(self, acceptor, la=20, limit=64, sample_size=24, steps=(20, 20), n_sample=48, forager=0, tolerance=0.02):
        self.acceptor, self.la, self.limit, self.sample_size, self.steps, self.n_sample = acceptor, la, limit, sample_size, steps, n_sample
        self.forager, self.tolerance = forager, tolerance
        self.anneal = acceptor == SA
        self.g = None

    def _graph(self):
        if self.g is None:
            from solverforge_amd import datasets

            g = datasets.make_graph(120, 500, 5, seed=11)
            g["colors"] = (datasets.stream(110, 120) % np.uint64(6)).astype(np.int64) - 1
            self.g = g
        return self.g

    def device(self, R, seed):
        import solverforge_amd as sfa

        d = sfa.build_graph_coloring(self._graph(), n_replicas=R)
        d.configure(sfa.SolverConfig(acceptor=self.acceptor, late_acceptance_size=self.la, forager=self.forager, accepted_count_limit=self.limit,
                                     random_seed=seed))
        _configure_acceptor(self, d, seed)
        return d

    def cpu(self, oracle, seed):
        g = self._graph()
        o = oracle.Model.graph_coloring(g["n_colors"], g["adj_off"], g["adj"], g["colors"])
        o.configure(acceptor=_oracle_acceptor(self.acceptor), la_size=self.la, forager=self.forager, limit=self.limit,
                    leaves=oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP, random_seed=seed)
        _configure_oracle_acceptor(self, o, seed)
        return o

    def device_state(self, d, r):
        return d.working_values(0, 0, replica=r).tolist()

    def cpu_state(self, o):
        return o.get_vars(0, 0).tolist()

    def path(self, d):
        model, gen = d.arith_flags()
        assert model["scalar_value_bytes"] == 1 and gen is None, (model, gen)  # the scalar engine ran, the generic one never


class _JobShop:
    """The two-class mixed job shop of test_gpu_mixed.py: scalar machine choice + machine sequences, BendableScore<2,1>, four leaves."""
    levels = 3
    block = False
    anneal = False
    env = {}
    steps = (20, 20)
    n_sample = 32

    def __init__(self):
        self.p = None

    def _problem(self):
        if self.p is None:
            from solverforge_amd import datasets

            p = datasets.make_jobshop(12, 5)
            n, m = p["n_ops"], 5
            r = datasets.stream(1, 3 * n)
            p["machine_idx"] = (r[:n] % np.uint64(m + 1)).astype(np.int64) - 1
            seqs = [[] for _ in range(m)]
            for op in range(n):
                where = int(r[n + op] % np.uint64(m + 2))
                if where < m:  # some operations stay unscheduled
                    seqs[where].append(op)
            p["sequences"] = seqs
            self.p = p
        return self.p

    def device(self, R, seed):
        import solverforge_amd as sfa

        d = sfa.build_jobshop(self._problem(), n_replicas=R, bendable=True)
        d.configure(sfa.SolverConfig(late_acceptance_size=24, accepted_count_limit=64, random_seed=seed))
        return d

    def cpu(self, oracle, seed):
        p = self._problem()
        o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=True)
        o.configure(la_size=24, limit=64, leaves=oracle.LEAF_LIST_CHANGE | oracle.LEAF_LIST_SWAP | oracle.LEAF_SCALAR_CHANGE | oracle.LEAF_SCALAR_SWAP,
                    random_seed=seed)
        return o

    def device_state(self, d, r):
        return d.working_values(0, 0, replica=r).tolist(), d.working_lists(1, r)

    def cpu_state(self, o):
        return o.get_vars(0, 0).tolist(), o.get_lists(1)

    def path(self, d):
        _, gen = d.arith_flags()
        assert gen is not None and gen["levels"] == 4 and gen["ruin"] == 0 and not gen["prec"] and gen["value_bytes"] == 2, gen


def _small_cvrp():
    from solverforge_amd import datasets

    return datasets.make_cvrp(60, 6, 40, seed=5)


def _sentinel_cvrp():
    """test_real_0xfffe_leg_meets_the_sentinel's model: 16-bit leg tables, not every leg finite, so no 32-bit deltas."""
    p = _top_problem(U16_LAST, n=40, v=4, seed=3)
    m, r0, r1 = p["matrix"], p["routes"][0], p["routes"][1]
    for a, b, val in [(r0[0], r0[1], UNREACHABLE), (r0[1], r0[2], -3), (r1[1], r1[2], UNREACHABLE), (r1[2], r1[3], U16_LAST), (r0[2], r1[0], UNREACHABLE)]:
        m[a, b] = m[b, a] = val
    return p


def _wave_mode(check):
    def path(d):
        got = d.wave_layout()
        assert check(*got), got
    return path


def _generic(**want):
    def path(d):
        _, gen = d.arith_flags()
        assert gen is not None and all(gen[k] == v for k, v in want.items()), (gen, want)
    return path


def _block_path(d):
    assert d.engine() == 1 and d.wave_layout()[0] == -1, (d.engine(), d.wave_layout())


CASES = {
    # wave engine (engine 2)
    "wave_compact": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, path=_wave_mode(lambda mode, renum: mode >= 3)),
    "wave_node_table": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, env={"SF_AMD_NODE_GLOBAL": "1", "SF_AMD_RENUMBER": "0"},
                                     path=_wave_mode(lambda mode, renum: mode == 6 and not renum)),
    "wave_node_table_renumbered": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, env={"SF_AMD_NODE_GLOBAL": "1", "SF_AMD_RENUMBER": "1"},
                                                path=_wave_mode(lambda mode, renum: mode == 6 and renum)),
    "wave_mode2": lambda: _Cvrp(lambda: _top_problem(U16_OUT), NEARBY, engine=2, path=_wave_mode(lambda mode, renum: mode == 2)),
    "wave_general": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, acceptor=0, limit=4, path=_wave_mode(lambda mode, renum: mode == 0)),
    # generic engine
    "generic_six_fast": lambda: _Cvrp(_small_cvrp, SIX_LEAVES, n_sample=24, path=_generic(fast=True, ring32=True, ruin=0)),
    "generic_seven_fast_ruin": lambda: _Cvrp(_small_cvrp, DEFAULT_POLICY, steps=(10, 10), n_sample=16,
                                             path=_generic(fast=True, node_global=True, ring32=True, ruin=3)),
    "generic_seven_general": lambda: _Cvrp(_sentinel_cvrp, DEFAULT_POLICY, ruin=(1, 6, 16), steps=(10, 10), n_sample=16, path=_generic(fast=False, ruin=2)),
    "generic_mixed_jobshop": _JobShop,
    # scalar engine
    "scalar_late_acceptance": lambda: _Graph(acceptor=1),
    "scalar_annealing": lambda: _Graph(acceptor=SA, limit=1, steps=(150, 150)),
    # block engine (engine 1)
    "block_two_leaf": lambda: _Cvrp(_small_cvrp, NEARBY, engine=1, block=True, path=_block_path),
    # SimulatedAnnealing on the list engines, fused: the per-replica temperature row and annealing stream.  On the oracle, calibration over
    # 128 samples under AcceptedCount(8) completes after 4 to 14 steps at the sampled seeds of a 256-CU and of a 304-CU device: far inside
    # the 60 steps (the test asserts it for its own sample), and for some replicas behind the first launch of 10, which then writes a
    # half-filled calibration back
    "wave_annealing": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, acceptor=SA, limit=8, sample_size=128, steps=(10, 50), n_sample=32,
                                    path=_wave_mode(lambda mode, renum: mode == 0)),
    "generic_annealing": lambda: _Cvrp(_small_cvrp, GENERIC_THREE, acceptor=SA, limit=8, sample_size=128, steps=(10, 50), n_sample=32, path=_generic(fast=False, ruin=0)),
    "block_annealing": lambda: _Cvrp(_small_cvrp, NEARBY, engine=1, acceptor=SA, limit=8, sample_size=128, steps=(10, 50), n_sample=32, block=True, path=_block_path),
    # DiversifiedLateAcceptance (the block engine refuses it): the per-replica history and its late-score bookkeeping
    "scalar_diversified": lambda: _Graph(acceptor=DLA, la=5, limit=8, n_sample=32),
    "wave_diversified": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, acceptor=DLA, la=5, limit=8, n_sample=32,
                                      path=_wave_mode(lambda mode, renum: mode == 0)),
    "generic_diversified": lambda: _Cvrp(_small_cvrp, GENERIC_THREE, acceptor=DLA, la=5, limit=8, n_sample=24, path=_generic(fast=False, ruin=0)),
}


# ---- the checks -------------------------------------------------------------------------------------------------------------------------
def _set_env(monkeypatch, case):
    for k in ("SF_AMD_NODE_GLOBAL", "SF_AMD_RENUMBER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def _start(case, R, seed):
    d = case.device(R, seed)
    d.set_step_seeds(None)  # check 4 needs seeds derived from random_seed + r: no explicit step seeds
    d.calculate_score()
    d.phase_start()
    return d


def _compare_replica(case, d, r, o, scores, best):
    """Check 1 for one replica: state, score, best score, counters (temperatures under SimulatedAnnealing)."""
    L = case.levels
    assert case.device_state(d, r) == case.cpu_state(o), r
    assert (scores[r] == o.score()[:L]).all(), (r, scores[r], o.score())
    assert (best[r] == o.best_score()[:L]).all(), (r, best[r], o.best_score())
    gst, ost = d.stats(r), o.stats()
    for k in COUNTERS:
        assert gst[k] == ost[k], (r, k, gst[k], ost[k])
    if case.anneal:
        gt, gc = d.annealing_state(r)
        ot, _, oc = o.annealing_state()
        assert gc == bool(oc), r
        assert (gt.view(np.uint64) == ot[:L].view(np.uint64)).all(), (r, gt, ot)


def _check_every_replica(d, scores, best):
    """Check 2."""
    fresh = d.fresh_score()
    assert (fresh == scores).all(), _rows_differ(fresh, scores)
    assert _lex_ge(best, scores).all(), np.flatnonzero(~_lex_ge(best, scores))[:8]


def _check_shift(scores, best, scores_b, best_b):
    """Check 4."""
    R = len(scores)
    assert (scores_b[:R - SHIFT] == scores[SHIFT:]).all(), _rows_differ(scores_b[:R - SHIFT], scores[SHIFT:])
    assert (best_b[:R - SHIFT] == best[SHIFT:]).all(), _rows_differ(best_b[:R - SHIFT], best[SHIFT:])


@pytest.mark.parametrize("name", list(CASES))
def test_large_launch(oracle, monkeypatch, name):
    case = CASES[name]()
    _set_env(monkeypatch, case)
    R, u = _launch_size(case.block)
    steps = sum(case.steps)
    d = _start(case, R, SEED)
    for n in case.steps:  # the second launch starts from state the first one wrote back
        d.solve_steps(n)
    case.path(d)
    scores, best = d.calculate_score().copy(), d.best_scores().copy()
    _check_every_replica(d, scores, best)
    assert d.total_stats()["step_count"] == R * steps  # check 3
    finals = []
    t0 = time.perf_counter()
    for r in _sample(R, u, case.n_sample):
        o = case.cpu(oracle, SEED + r)
        o.phase_start()
        o.steps(steps)
        _compare_replica(case, d, r, o, scores, best)
        if case.anneal:
            assert not o.annealing_state()[2], r  # the calibration completed inside the run
        finals.append(repr(case.cpu_state(o)))
    print(f"{name}: R={R} sample={len(finals)} oracle+compare {time.perf_counter() - t0:.2f} s")
    assert len(set(finals)) == len(finals)  # check 5
    d.close()
    b = _start(case, R, SEED + SHIFT)
    for n in case.steps:
        b.solve_steps(n)
    _check_shift(scores, best, b.calculate_score(), b.best_scores())
    b.close()


BUDGET_CASES = {
    "wave": lambda: _Cvrp(_small_cvrp, NEARBY, engine=2, la=7, limit=16, path=_wave_mode(lambda mode, renum: mode >= 3)),
    "generic": lambda: _Cvrp(_small_cvrp, ("nearby_change", "nearby_swap", "sublist_change", "list_reverse", "kopt"), la=7, limit=16, n_sample=24,
                             path=_generic(fast=True, ruin=0)),
}


@pytest.mark.parametrize("name", list(BUDGET_CASES))
def test_move_budgeted_launch_at_size(oracle, monkeypatch, name):
    """sf_solve_moves: every replica runs whole steps until it has pulled its own budget of candidates, so replicas of one launch stop after
    different step counts.  Each sampled replica is the oracle advanced by the step count that replica reports, after each of two launches;
    the budget is per replica, so check 4 holds as it stands."""
    case = BUDGET_CASES[name]()
    _set_env(monkeypatch, case)
    R, u = _launch_size(False)
    budgets = (400, 900)
    d = _start(case, R, SEED)
    sample = _sample(R, u, case.n_sample)
    oracles = {}
    for r in sample:
        oracles[r] = case.cpu(oracle, SEED + r)
        oracles[r].phase_start()
    done = dict.fromkeys(sample, 0)
    for launch, budget in enumerate(budgets):
        d.solve_moves(10_000, budget)
        scores, best = d.calculate_score().copy(), d.best_scores().copy()
        for r in sample:
            n = d.stats(r)["step_count"]
            assert n > done[r], (launch, r)
            oracles[r].steps(n - done[r])
            done[r] = n
            _compare_replica(case, d, r, oracles[r], scores, best)
    case.path(d)
    _check_every_replica(d, scores, best)
    # the launches ended on the budget, not on max_steps, and replicas got different distances
    assert max(done.values()) < 10_000 and len(set(done.values())) > 1, sorted(set(done.values()))
    finals = [repr(case.cpu_state(o)) for o in oracles.values()]
    assert len(set(finals)) == len(finals)
    d.close()
    b = _start(case, R, SEED + SHIFT)
    for budget in budgets:
        b.solve_moves(10_000, budget)
    _check_shift(scores, best, b.calculate_score(), b.best_scores())
    b.close()


def test_migrate_local_at_size():
    """sf_portfolio_migrate_local over several residencies: n_elite 64, n_replace R / 4, after a run with a short LateAcceptance history
    (best scores tie in places).  The ranking rule restated in numpy -- descending best score, ties to the lower index, adopter i (from the
    bottom) takes elite i % n_elite, an adopter that already holds its elite's score is skipped -- decides from the bulk arrays what every
    row must hold afterwards."""
    case = _Cvrp(_small_cvrp, NEARBY, la=20, limit=40, path=_wave_mode(lambda mode, renum: mode >= 3))
    R, u = _launch_size(False)
    d = _start(case, R, SEED)
    for n in (20, 20):
        d.solve_steps(n)
    case.path(d)
    scores0, best0 = d.calculate_score().copy(), d.best_scores().copy()
    assert len(np.unique(best0, axis=0)) < R  # ties exist: the stable order matters
    order = np.lexsort((-best0[:, 1], -best0[:, 0]))  # stable: ties to the lower index
    assert all(tuple(best0[order[i]]) >= tuple(best0[order[i + 1]]) and (tuple(best0[order[i]]) > tuple(best0[order[i + 1]]) or order[i] < order[i + 1])
               for i in range(R - 1))
    n_elite, n_replace = 64, R // 4
    i = np.arange(n_replace)
    adopters, elites = order[R - 1 - i], order[i % n_elite]
    takes = (best0[adopters] != best0[elites]).any(axis=1)
    adopters, elites = adopters[takes], elites[takes]
    assert len(adopters) > n_replace // 2
    spot = np.random.default_rng(7).choice(len(adopters), size=8, replace=False)
    elite_lists = {int(elites[k]): d.working_lists(0, int(elites[k]), best=True) for k in spot}
    adopted = d.migrate_local(n_elite, n_replace)
    assert adopted == len(adopters)
    scores1, best1 = d.calculate_score().copy(), d.best_scores().copy()
    want_scores, want_best = scores0.copy(), best0.copy()
    want_scores[adopters] = best0[elites]
    want_best[adopters] = best0[elites]
    assert (scores1 == want_scores).all(), _rows_differ(scores1, want_scores)  # adopters hold their elite's best score, every other row is unchanged
    assert (best1 == want_best).all(), _rows_differ(best1, want_best)
    fresh = d.fresh_score()
    assert (fresh == scores1).all(), _rows_differ(fresh, scores1)
    for k in spot:
        a, e = int(adopters[k]), int(elites[k])
        assert d.working_lists(0, a) == elite_lists[e] and d.working_lists(0, a, best=True) == elite_lists[e], (a, e)
    d.solve_steps(10)  # the search continues from the adopted states
    scores2 = d.calculate_score()
    assert (d.fresh_score() == scores2).all()
    assert _lex_ge(d.best_scores(), scores2).all()
    d.close()
