"""GPU: the acceptors that keep a state row per replica on the device -- TabuSearch (stamp tables and rings in a per-replica arena),
GreatDeluge (water level) and StepCountingHillClimbing (best step score, count) -- at launches of several residencies.

tests/test_gpu_tabu.py and tests/test_gpu_acceptors.py check that state candidate by candidate against their mirrors, in contexts of 3
replicas.  A state row is what goes wrong past index 0, past lane 63 and at a residency boundary, and every wall-clock solve runs tens
of thousands of replicas; so here every site runs one configuration (`all_four`, `gd_first`, `sc_first`) with the launch size and the
sample of tests/test_gpu_large_launch.py: R = 2 * 32 * CUs + 37 (block engine: 2 * 2 * CUs + 5), and the replicas 0, 1, 3, 4, 5, 63, 64,
u - 1, u, 2u - 1, 2u, R - 5, R - 2, R - 1 (those 14 and no further draw: a traced reference costs far more than an oracle run).  The oracle cannot run these acceptors, so the verdict comes from the
mirror-checked traced runs of the two feature tests (every accept flag is the mirror's, every score the oracle model's, the state after
every step the mirror's):

  1. context A (R replicas, random_seed SEED, two fused launches): every sampled replica r ends in the snapshot -- score, best score,
     working state, the seven counters, acceptor / tabu state -- of a traced run in a context of ONE replica seeded SEED + r.  The
     traced run anchors that context; the equality carries its verdict to index r of the large launch;
  2. one anchor in place, which does not lean on "replica r is a function of random_seed + r": in A's twin the last replica, R - 1, is
     traced directly at size for the same steps, against a mirror and an oracle model of its own; the twin then holds A's snapshots;
  3. every replica: incremental score == full recalculation, best score >= score, the step counters sum to R * steps;
  4. shift invariance: context B seeded SEED + 5 gives scores_B[:R - 5] == scores_A[5:], best scores likewise, and for the sampled
     r >= 5 the acceptor / tabu state of B at r - 5 is A's at r;
  5. on the references alone: over the sampled replicas the mirrors showed the events that tell the rule from its neighbours (EVENTS:
     the state mattered), and the references end in pairwise distinct working states.

Each case asserts the kernel path it took.  Steps: 20 + 20 under GreatDeluge and StepCounting, as in the feature test; under TabuSearch
12 + 12 (scalar), 16 + 16 (wave), 10 + 10 (generic, mixed), from a measurement on a 256-CU device over these seeds of the first step
(from 0) that shows an event: 0 for the GreatDeluge events, 2 to 4 for the StepCounting events; under TabuSearch 8 or less for all but
the refusal by the move memory alone, which first shows at step 29 at the wave site (replica 0), 17 at the generic site (replica 63)
and 8 at the mixed site (replica 1; see _Tabu for the scalar site).  Those replicas are in the sample whatever the CU count.

A last test reuses a dirty tabu arena under another policy: tabu_phase_rows keeps the allocation when the new policy needs no more
room and derives every replica's address from the new row size, so the second phase of a 3-replica context is traced at replicas 0 and
2 against a fresh mirror, once from the large policy to a small one (arena kept) and once the other way (arena reallocated)."""
import time

import pytest

import tabu_mirror as tm
import test_gpu_acceptors as ac
import test_gpu_tabu as tb
from test_gpu_large_launch import SHIFT, _launch_size, _lex_ge, _rows_differ, _sample

pytestmark = pytest.mark.gpu

SEED = 7_000  # replica r of context A runs random_seed SEED + r
N_SAMPLE = 14  # the mandatory indices alone: the traced references are the cost of a case
EVENTS = {
    "tabu": tuple("refused_by_%s_alone" % m for m in tm.MEMORIES) + ("admissible_again_after_eviction",),
    "gd_first": ("accepted_through_water_only", "refused_below_water"),
    "sc_first": ("since_reached_limit", "since_reset_afterwards"),
}


def _scalar_path(d):
    model, gen = d.arith_flags()
    assert model["scalar_value_bytes"] != 0 and gen is None, (model, gen)  # the scalar engine ran, the generic one never


def _wave_path(d):
    assert d.wave_layout()[0] == 0, d.wave_layout()  # the general replay, never a FAST kernel


def _generic_path(d):
    _, gen = d.arith_flags()
    assert gen is not None and not gen["fast"], gen


def _block_path(d):
    assert d.engine() == 1, d.engine()


PATHS = {"scalar": _scalar_path, "wave": _wave_path, "generic": _generic_path, "mixed": _generic_path, "block": _block_path}


class _Tabu:
    """TabuSearch with all four memories at a site of tests/test_gpu_tabu.py.

    The scalar site cannot show a refusal by the move memory alone under this policy, and is not asked for one.  A scalar swap's
    identity is its own undo identity, so under equal move and undo tenures the undo memory holds whatever the move memory holds.  A
    scalar change (e, from, to) can be proposed again only once e holds `from` again: the direct way back is the move whose undo
    identity is (e, from, to), which the undo memory then keeps longer than the move memory keeps the original; the way round over a
    third value takes two aspirational accepts of a tabu entity inside six steps.  Measured: no such refusal in 500 steps at any of
    the 16 sampled seeds of a 256-CU device, while the list sites show it (wave: replica 0 at step 29; generic: replica 63 at step 17,
    replica R - 5 at step 36; mixed: 14 of 16 replicas by step 41).  The move ring of the scalar site is still compared word for word
    with the mirror's after every traced step and in every snapshot."""
    # two launches; chosen per site from the measured first step of the last required event (see the module docstring), with a margin
    STEPS = {"scalar": (12, 12), "wave": (16, 16), "generic": (10, 10), "mixed": (10, 10)}

    def __init__(self, site):
        self.site, self.steps = site, self.STEPS[site]
        self.policy, self.forager, self.limit, self.leaves = tb.SITE_CONFIGS[site]["all_four"]
        assert all(t is not None for t in self.policy[:4])
        self.events = tuple(e for e in EVENTS["tabu"] if not (site == "scalar" and e == "refused_by_move_alone"))

    def device(self, oracle, n_replicas, seed):
        d = tb._build(self.site, n_replicas=n_replicas, leaves=self.leaves[self.site])
        d.set_step_seeds(None)  # seeds derived from random_seed + r: no explicit step seeds
        tb._configure(d, self.policy, self.forager, self.limit, seed=seed)
        return d

    def trace(self, oracle, d, replica, steps):
        return tb.trace_replica(oracle, d, self.site, self.policy, replica, steps)

    def snapshot(self, d, replicas):
        return tb._snapshot(d, self.site, replicas)

    def state(self, d, r):
        return tb._tabu_tuple(d, r)


class _Acceptor:
    """GreatDeluge / StepCounting under FirstAccepted at a site of tests/test_gpu_acceptors.py."""
    steps = (20, 20)

    def __init__(self, site, run):
        self.site, self.events = site, EVENTS[run]
        self.acceptor, self.param, self.forager, self.limit = ac.TRACE[run]

    def device(self, oracle, n_replicas, seed):
        d = ac._build(self.site, n_replicas=n_replicas)
        d.set_step_seeds(None)
        ac._configure(d, self.acceptor, self.param, self.forager, self.limit, ac._site_cfg(oracle, self.site)[0], seed)
        return d

    def trace(self, oracle, d, replica, steps):
        return ac.trace_replica(oracle, d, self.site, self.acceptor, self.param, replica, steps)

    def snapshot(self, d, replicas):
        return ac._snapshot(d, self.site, True, replicas)

    def state(self, d, r):
        return ac._acceptor_tuple(d, r)


CASES = {"tabu-" + site: (lambda site=site: _Tabu(site)) for site in tb.SITES}
CASES.update({run + "-" + site: (lambda site=site, run=run: _Acceptor(site, run)) for run in ("gd_first", "sc_first") for site in ac.SITES})


def _fused(case, oracle, n_replicas, seed):
    d = case.device(oracle, n_replicas, seed)
    for n in case.steps:  # the second launch starts from state the first one wrote back
        d.solve_steps(n)
    return d


@pytest.mark.parametrize("name", list(CASES))
def test_state_rows_at_size(oracle, name):
    case = CASES[name]()
    R, u = _launch_size(case.site == "block")
    steps = sum(case.steps)
    sample = _sample(R, u, N_SAMPLE)
    a = _fused(case, oracle, R, SEED)
    PATHS[case.site](a)
    scores, best = a.calculate_score().copy(), a.best_scores().copy()
    got = case.snapshot(a, sample)  # fresh_score() == calculate_score() over all replicas is asserted inside
    states = {r: case.state(a, r) for r in sample}
    assert _lex_ge(best, scores).all(), _rows_differ(best, scores)
    assert a.total_stats()["step_count"] == R * steps
    a.close()
    # 1. every sampled replica against the traced run of a one-replica context
    t0 = time.perf_counter()
    seen, finals = set(), []
    for r, snap in zip(sample, got):
        d = case.device(oracle, 1, SEED + r)
        seen |= set(case.trace(oracle, d, 0, steps))
        assert case.snapshot(d, [0])[0] == snap, r
        finals.append(repr(snap[2]))
        d.close()
    print(f"{name}: R={R} sample={len(sample)} steps={steps} traced references {time.perf_counter() - t0:.2f} s; events {sorted(seen)}")
    # 5. the references: the state mattered, and no two trajectories coincide
    assert not [e for e in case.events if e not in seen], sorted(seen)
    assert len(set(finals)) == len(finals)
    # 2. the last replica traced in place
    t0 = time.perf_counter()
    twin = case.device(oracle, R, SEED)
    in_place = case.trace(oracle, twin, R - 1, steps)
    print(f"{name}: replica {R - 1} in place {time.perf_counter() - t0:.2f} s; events {sorted(in_place)}")
    assert case.snapshot(twin, sample) == got
    twin.close()
    # 4. shift invariance, the state rows included
    b = _fused(case, oracle, R, SEED + SHIFT)
    scores_b, best_b = b.calculate_score(), b.best_scores()
    assert (scores_b[:R - SHIFT] == scores[SHIFT:]).all(), _rows_differ(scores_b[:R - SHIFT], scores[SHIFT:])
    assert (best_b[:R - SHIFT] == best[SHIFT:]).all(), _rows_differ(best_b[:R - SHIFT], best[SHIFT:])
    for r in sample:
        if r >= SHIFT:
            assert case.state(b, r - SHIFT) == states[r], r
    b.close()


SMALL_POLICY = [None, None, 5, None, True]  # the move ring alone: a row of far fewer words than the four memories' row
PHASE_STEPS = (10, 30)  # the second phase: long enough for its memories to refuse at every site (the scalar site needs 25 steps)


@pytest.mark.parametrize("order", ["arena_kept", "arena_grows"])
@pytest.mark.parametrize("site", tb.SITES)
def test_a_dirty_arena_under_another_policy(oracle, site, order):
    large, forager, limit, leaves = tb.SITE_CONFIGS[site]["all_four"]
    first, second = (large, SMALL_POLICY) if order == "arena_kept" else (SMALL_POLICY, large)
    seen, snaps = set(), []
    for r in (0, 2):  # a traced launch moves every replica: one context per traced replica
        d = tb._build(site, leaves=leaves[site])
        tb._configure(d, first, forager, limit)
        d.solve_steps(PHASE_STEPS[0])
        pushes = [d.tabu_state(k)["pushes"] for k in range(tb.R)]
        assert all(p[i] > 0 for p in pushes for i, t in enumerate(first[:4]) if t is not None), pushes  # the arena is dirty
        d.configure_tabu(*second)
        d.phase_start()
        o = tb._oracle_model(oracle, site, tb._state(d, site, r))  # the replica's working solution after the first phase
        seen |= set(tb.trace_replica(oracle, d, site, second, r, PHASE_STEPS[1], o=o))
        snaps.append(tb._snapshot(d, site))
        d.close()
    print(f"{site} {order}: events of the second phase {sorted(seen)}")
    assert snaps[0] == snaps[1]
    assert len({str(s[2]) for s in snaps[0]}) == tb.R
    # the second phase's memories refused something: the move ring alone, or the entity stamps of the row that has just grown
    assert ("refused_by_move_alone" if order == "arena_kept" else "refused_by_entity_alone") in seen, sorted(seen)
