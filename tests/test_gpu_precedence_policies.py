"""GPU: the precedence engine (the PREC instantiations of k_mixed_search_wave) under every acceptor and forager the host admits on a
precedence model.  tests/test_gpu_precedence*.py and tests/test_gpu_prec_placement.py cover placements, group widths, residencies and
construction under LateAcceptance alone; here the policy varies and the placements are three: `lds` (grouped trial evaluator at its
default T), `lds_one_trial` (every trial applied, evaluated and undone) and `hbm` (Kahn scratch in HBM; with the two plain list leaves and
no slot policy: the 64-lane trial sweep).  Every fused launch's placement is asserted.

The rule no other engine has: a multi-swap of the critical-path leaf carries Move::requires_score_improvement (evaluation.rs:95-113).  It
is scored and counted and reaches the acceptor only if it beats the last step score -- whatever the acceptor.  A kernel that consulted
the acceptor for a gated multi-swap would spend a draw under SimulatedAnnealing (and shift every later decision), record a calibration
sample, or let a candidate through the water level of GreatDeluge.  So every acceptor must meet, in at least one of its runs, a gated
multi-swap that the acceptor ON ITS OWN would have accepted (judged on the reference side: the oracle's flag 16 and a restatement of the
acceptor).  HillClimbing cannot show one: it accepts `sc > cur` only, which is the gate's own condition.

1. Acceptors the oracle runs itself, bit for bit (PART1, the table below): traced steps (records, scores, flags incl. the gate bit, the
   applied move, the seven counters, the lists, the annealing temperatures after every step), then the same configuration fused with
   three replicas (seed + r) as two launches and as one budgeted launch, against the oracle's own run of every replica.
   (DiversifiedLateAcceptance has no state getter in the C ABI: its history and best show in the decisions of the following steps
   and in the fused end states.  sf_get_annealing_state reports the temperatures and the calibration flag, not the generator's words: a
   shifted draw stream shows in the steps after it, which is why the SA run that meets the gate must go on.)

   acceptor                          forager                     union    shop  start      placement
   HillClimbing                      AcceptedCount(1)            leaf     6x4   scheduled  lds
   HillClimbing                      AcceptedCount(7)            four     10x5  shuffled   lds_one_trial
   HillClimbing                      AcceptedCount(70)           policy   6x4   cyclic     hbm
   HillClimbing                      FirstAccepted               four     6x4   shuffled   hbm
   HillClimbing                      BestScore                   leaf     6x4   shuffled   lds_one_trial
   HillClimbing                      FirstBestScoreImproving     policy   6x4   scheduled  lds
   HillClimbing                      FirstLastStepScoreImproving four     6x4   cyclic     lds
   HillClimbing                      AcceptedCount(7)            plain    6x4   shuffled   hbm (sweep)
   SimulatedAnnealing(T 2, 6)        AcceptedCount(1)            four     6x4   shuffled   lds
   SimulatedAnnealing(calibrated 12) AcceptedCount(7)            leaf     6x4   shuffled   lds_one_trial
   SimulatedAnnealing(T 2, 6)        AcceptedCount(70)           four     6x4   scheduled  hbm
   SimulatedAnnealing(calibrated 12) FirstAccepted               policy   6x4   shuffled   lds
   SimulatedAnnealing(T 2, 6)        BestScore                   leaf     6x4   scheduled  hbm
   SimulatedAnnealing(calibrated 12) FirstBestScoreImproving     four     10x5  scheduled  lds_one_trial
   SimulatedAnnealing(T 2, 6)        FirstLastStepScoreImproving policy   6x4   cyclic     lds_one_trial
   SimulatedAnnealing(T 2, 6)        AcceptedCount(7)            plain    6x4   scheduled  hbm (sweep)
   DiversifiedLateAcceptance(0.0)    AcceptedCount(1)            policy   6x4   shuffled   lds_one_trial
   DiversifiedLateAcceptance(0.01)   AcceptedCount(7)            four     6x4   scheduled  hbm
   DiversifiedLateAcceptance(0.5)    AcceptedCount(70)           leaf     6x4   shuffled   lds
   DiversifiedLateAcceptance(0.0)    FirstAccepted               leaf     6x4   scheduled  hbm
   DiversifiedLateAcceptance(0.01)   BestScore                   four     6x4   cyclic     lds
   DiversifiedLateAcceptance(0.5)    FirstBestScoreImproving     policy   6x4   shuffled   hbm
   DiversifiedLateAcceptance(0.01)   FirstLastStepScoreImproving four     10x5  shuffled   lds
   DiversifiedLateAcceptance(0.5)    AcceptedCount(7)            plain    10x5  shuffled   hbm (sweep)
   LateAcceptance (control)          AcceptedCount(7)            four     6x4   shuffled   lds

   and, outside the table, SimulatedAnnealing(T 0.5, 2, 6) and DiversifiedLateAcceptance(0.01) under AcceptedCount(7) on the 6 x 4 mixed
   job shop with durations (three score levels: the four-level kernels) with the leaf, permute and the plain list and scalar pairs.

   unions: leaf = ("precedence",); four = ("precedence", "permute", "list_change", "list_swap"); policy = POLICY_LEAVES of
   tests/test_gpu_precedence_leaf.py with the slot's precedence policy (route-graph filter, ruin leaf with the hooks); plain =
   ("list_change", "list_swap") without the policy, under hbm the only route into the trial sweep (prec_sweep asserted).
2. GreatDeluge and StepCountingHillClimbing: the two exact equivalences of tests/test_gpu_acceptors.py on the `four` union, and traced
   runs at replicas 0 and 2 against tests/acceptor_mirror.py with consult = doable and not (multi-swap and sc <= cur); fused runs end
   where the traced run did.
3. TabuSearch on the plain union of the shop and on the mixed job shop with the makespan objective, against tests/tabu_mirror.py; a
   union with the critical-path leaf is refused.
4. Variable Neighborhood Descent (to its end: a local optimum by the oracle) and LimitedNeighborhood (a child limit of 65 under
   RoundRobin, a root limit of 64 under StratifiedRandom) on the plain union.
5. MODE 2 (more than 2,048 replicas, grouped evaluator off: `prec_occ`) under HillClimbing, SimulatedAnnealing and
   DiversifiedLateAcceptance.

The conditions on the inputs (the gate binds, SA draws are spent behind it, the six events of GreatDeluge / StepCounting, a step of
more than 64 candidates under AcceptedCount(70), the sweep, the tabu refusals and an eviction) are asserted from the reference side;
seeds and starts were picked by running the oracle and the mirrors alone."""
import numpy as np
import pytest

import acceptor_mirror as am
import limited_mirror as lm
import tabu_mirror as tm
import test_gpu_acceptors as ta
import test_gpu_tabu as tt
import vnd_mirror as vm
from test_gpu_precedence_leaf import BITS, COUNTERS, POLICY_LEAVES, _assert_placement, _shuffled, _t

pytestmark = pytest.mark.gpu

HC, LA, SA, DLA, GD, SC = 0, 1, 3, 4, 5, 6
AC, FA, BS, FBSI, FLSI = 0, 1, 2, 3, 4
MULTI_SWAP = 10  # SF_MOVE_LIST_MULTI_SWAP
GATED = 16  # the oracle's flag of a candidate turned away by requires_score_improvement
R = 3
LA_SIZE = 4
RUIN = (2, 5, 4)
ENV = {"lds": None, "lds_one_trial": ("SF_AMD_PREC_GROUPS", "0"), "hbm": ("SF_AMD_PREC_HBM", "1")}
UNIONS = {"leaf": (("precedence",), False), "four": (("precedence", "permute", "list_change", "list_swap"), False), "policy": (POLICY_LEAVES, True),
          "plain": (("list_change", "list_swap"), False)}
SHOPS = {"6x4": (6, 4, 3), "10x5": (10, 5, 2)}
_memo = {}


def _place(monkeypatch, mode):
    """The environment of a placement, set before the director is built and cleared when the test ends."""
    if ENV[mode]:
        monkeypatch.setenv(*ENV[mode])
    return mode


def _problem(shop, start):
    """scheduled: the generator's schedule; shuffled: a few operations on the machine of their job predecessor (_shuffled: intra-list
    moves close cycles); cyclic: those sequences reversed -- job successors in front of their predecessors, hard-level penalties."""
    from solverforge_amd import datasets

    jobs, machines, seed = SHOPS[shop]
    p = datasets.make_precedence_shop(jobs, machines, seed=seed)
    if start != "scheduled":
        p, _ = _shuffled(p, 1)
    if start == "cyclic":
        p["sequences"] = [list(reversed(s)) for s in p["sequences"]]
    return p


def _check_placement(d, mode, p, union):
    leaves, policy = UNIONS[union]
    ruin = "ruin" in leaves
    _assert_placement(d, mode, p, tables=policy or ruin or "precedence" in leaves, ruin_inst=ruin)


def _score(x, levels=2):
    return tuple(int(v) for v in x[:levels])


# ---- restatements of the acceptors of part 1, to say what the acceptor ALONE would do with a gated candidate --------------------------------
class _Hill:
    def phase_started(self, cur):
        pass

    def is_accepted(self, cur, sc):
        return sc > cur

    would_accept = is_accepted

    def step_ended(self, cur):
        pass


class _Late(_Hill):
    """late_acceptance.rs:89-125 (every slot filled at the phase start)."""

    def __init__(self, size):
        self.size = size

    def phase_started(self, cur):
        self.history, self.at = [cur] * self.size, 0

    def is_accepted(self, cur, sc):
        return sc >= cur or sc >= self.history[self.at]

    would_accept = is_accepted

    def step_ended(self, cur):
        self.history[self.at] = cur
        self.at = (self.at + 1) % self.size


class _Diversified(_Late):
    """diversified_late_acceptance.rs:118-176: + within |best| x tolerance (per level, rounded half away from zero) of the best step score."""

    def __init__(self, size, tolerance):
        self.size, self.tolerance = size, tolerance

    def phase_started(self, cur):
        _Late.phase_started(self, cur)
        self.best = cur

    def is_accepted(self, cur, sc):
        if _Late.is_accepted(self, cur, sc):
            return True
        return sc >= tuple(am.wrap(b - am.multiply_level(am.wrap(-b) if b < 0 else b, self.tolerance)) for b in self.best)

    would_accept = is_accepted

    def step_ended(self, cur):
        if cur > self.best:
            self.best = cur
        _Late.step_ended(self, cur)


class _Annealing:
    """The oracle's stand-alone SimulatedAnnealingAcceptor follows the run: is_accepted for every consulted candidate (a draw may be
    spent, a calibration sample recorded).  would_accept(cur, sc) must not disturb it: a second acceptor is brought to the same state by
    replaying the log and asked alone.  It answers True only for an acceptance by a favourable draw."""

    def __init__(self, oracle, seed, anneal):
        self.oracle, self.kw = oracle, dict(anneal, levels=2, hard_levels=1, seed=seed)
        self.live, self.log = oracle.Annealer(**self.kw), []

    @staticmethod
    def _pad(sc):
        return list(sc) + [0] * (4 - len(sc))

    def phase_started(self, cur):
        self.live.phase_started()
        self.log.append(("phase",))

    def is_accepted(self, cur, sc):
        self.log.append(("ask", cur, sc))
        return self.live.is_accepted(self._pad(cur), self._pad(sc))[0]

    def step_ended(self, cur):
        self.live.step_ended()
        self.log.append(("end",))

    def would_accept(self, cur, sc):
        if sc >= cur:
            return False  # accepted without a draw: nothing a wrongly consulted candidate would shift
        a = self.oracle.Annealer(**self.kw)
        i = 0
        while i < len(self.log):
            op = self.log[i]
            if op[0] == "phase":
                a.phase_started()
            elif op[0] == "end":
                a.step_ended()
            else:
                j = i
                while j < len(self.log) and self.log[j][0] == "ask" and self.log[j][1] == op[1]:
                    j += 1
                a.is_accepted_many(self._pad(op[1]), [self._pad(x[2]) for x in self.log[i:j]])
                i = j - 1
            i += 1
        accepted, drew, _, _ = a.is_accepted(self._pad(cur), self._pad(sc))
        return accepted and drew


# ---- part 1 -----------------------------------------------------------------------------------------------------------------------------------
T_EXPLICIT = dict(mode=1, temperatures=(2.0, 6.0), decay_rate=0.97)
T_CALIBRATED = dict(mode=2, sample_size=12, target_probability=0.6)
T_EXPLICIT3 = dict(mode=1, temperatures=(0.5, 2.0, 6.0), decay_rate=0.97)  # the mixed job shop: two hard levels, then the makespan


def _row(acceptor, param, forager, limit, union, shop, start, placement, seed, steps=10):
    return dict(acceptor=acceptor, param=param, forager=forager, limit=limit, union=union, shop=shop, start=start, placement=placement, seed=seed, steps=steps)


PART1 = {
    "hc_ac1": _row(HC, None, AC, 1, "leaf", "6x4", "scheduled", "lds", 11),
    "hc_ac7": _row(HC, None, AC, 7, "four", "10x5", "shuffled", "lds_one_trial", 12, steps=4),
    "hc_ac70": _row(HC, None, AC, 70, "policy", "6x4", "cyclic", "hbm", 13, steps=5),
    "hc_first": _row(HC, None, FA, 0, "four", "6x4", "shuffled", "hbm", 14),
    "hc_best": _row(HC, None, BS, 0, "leaf", "6x4", "shuffled", "lds_one_trial", 15, steps=6),
    "hc_fbsi": _row(HC, None, FBSI, 0, "policy", "6x4", "scheduled", "lds", 16, steps=6),
    "hc_flsi": _row(HC, None, FLSI, 0, "four", "6x4", "cyclic", "lds", 17),
    "hc_sweep": _row(HC, None, AC, 7, "plain", "6x4", "shuffled", "hbm", 18),
    "sa_ac1": _row(SA, T_EXPLICIT, AC, 1, "four", "6x4", "shuffled", "lds", 21, steps=16),
    "sa_cal_ac7": _row(SA, T_CALIBRATED, AC, 7, "leaf", "6x4", "shuffled", "lds_one_trial", 22, steps=14),
    "sa_ac70": _row(SA, T_EXPLICIT, AC, 70, "four", "6x4", "scheduled", "hbm", 23),
    "sa_cal_first": _row(SA, T_CALIBRATED, FA, 0, "policy", "6x4", "shuffled", "lds", 24, steps=20),
    "sa_best": _row(SA, T_EXPLICIT, BS, 0, "leaf", "6x4", "scheduled", "hbm", 25, steps=6),
    "sa_cal_fbsi": _row(SA, T_CALIBRATED, FBSI, 0, "four", "10x5", "scheduled", "lds_one_trial", 26, steps=4),
    "sa_flsi": _row(SA, T_EXPLICIT, FLSI, 0, "policy", "6x4", "cyclic", "lds_one_trial", 27, steps=5),
    "sa_sweep": _row(SA, T_EXPLICIT, AC, 7, "plain", "6x4", "scheduled", "hbm", 28),
    "dla0_ac1": _row(DLA, 0.0, AC, 1, "policy", "6x4", "shuffled", "lds_one_trial", 31),
    "dla1_ac7": _row(DLA, 0.01, AC, 7, "four", "6x4", "scheduled", "hbm", 32),
    "dla50_ac70": _row(DLA, 0.5, AC, 70, "leaf", "6x4", "shuffled", "lds", 33),
    "dla0_first": _row(DLA, 0.0, FA, 0, "leaf", "6x4", "scheduled", "hbm", 34),
    "dla1_best": _row(DLA, 0.01, BS, 0, "four", "6x4", "cyclic", "lds", 35, steps=6),
    "dla50_fbsi": _row(DLA, 0.5, FBSI, 0, "policy", "6x4", "shuffled", "hbm", 36, steps=4),
    "dla1_flsi": _row(DLA, 0.01, FLSI, 0, "four", "10x5", "shuffled", "lds", 37),
    "dla50_sweep": _row(DLA, 0.5, AC, 7, "plain", "10x5", "shuffled", "hbm", 38),
    "la_control": _row(LA, None, AC, 7, "four", "6x4", "shuffled", "lds", 41),
}
FUSED_EXTRA = 4  # fused runs go this many steps past the traced ones


def _table_is_complete():
    rows = list(PART1.values())
    foragers = {(AC, 1), (AC, 7), (AC, 70), (FA, 0), (BS, 0), (FBSI, 0), (FLSI, 0)}
    for a in (HC, SA, DLA):
        mine = [c for c in rows if c["acceptor"] == a]
        assert {(c["forager"], c["limit"]) for c in mine} == foragers, a
        assert {c["union"] for c in mine} == set(UNIONS) and {c["placement"] for c in mine} == set(ENV), a
    assert {c["param"]["mode"] for c in rows if c["acceptor"] == SA} == {1, 2}
    assert {c["param"] for c in rows if c["acceptor"] == DLA} == {0.0, 0.01, 0.5}
    assert sum(c["acceptor"] == LA for c in rows) == 1
    assert all(c["placement"] == "hbm" for c in rows if c["union"] == "plain")


def _oracle_shop(oracle, p, union, seed, acceptor=LA, param=None, forager=AC, limit=7, la=LA_SIZE, random_ties=True):
    leaves, policy = UNIONS[union]
    o = oracle.Model.precedence_shop(p["durations"], p["successors"], p["sequences"], p["expected_owner"])
    o.configure(acceptor=0 if acceptor == HC else 1, la_size=la, forager=forager, limit=limit, leaves=sum(BITS[x] for x in leaves), random_seed=seed,
                random_ties=random_ties)
    o.set_ruin(*RUIN)
    o.set_kopt(1, 0)
    o.set_precedence_policy(policy)
    if acceptor == SA:
        o.configure_annealing(levels=2, hard_levels=1, seed=seed, **param)
    if acceptor == DLA:
        o.configure_diversified(la, param)
    return o


def _device_shop(p, union, seed, acceptor=LA, param=None, forager=AC, limit=7, la=LA_SIZE, n_replicas=R, random_ties=True):
    import solverforge_amd as sfa

    leaves, policy = UNIONS[union]
    d = sfa.build_precedence_shop(p, n_replicas=n_replicas, leaves=leaves, ruin=RUIN, precedence_policy=policy)
    d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=la, forager=forager, accepted_count_limit=limit, random_seed=seed,
                                 random_ties=random_ties))
    if acceptor == SA:
        kw = dict(param)
        d.configure_annealing(mode=kw.pop("mode"), temperatures=kw.pop("temperatures", ()), decay_rate=kw.pop("decay_rate", 0.999985),
                              calibration_sample_size=kw.pop("sample_size", 128), target_acceptance_probability=kw.pop("target_probability", 0.80), seed=seed)
        assert not kw
    if acceptor == DLA:
        d.configure_diversified(param)
    return d


def _mirror_of(oracle, c, seed):
    if c["acceptor"] == HC:
        return _Hill()
    if c["acceptor"] == LA:
        return _Late(LA_SIZE)
    if c["acceptor"] == DLA:
        return _Diversified(LA_SIZE, c["param"])
    return _Annealing(oracle, seed, c["param"])


def _anneal_words(o):
    t, _, calibrating = o.annealing_state()
    return t[:2].view(np.uint64).tolist(), bool(calibrating)


def _end_of(o, c):
    st = o.stats()
    return (_score(o.score()), _score(o.best_score()), o.get_lists(0), [st[k] for k in COUNTERS], _anneal_words(o) if c["acceptor"] == SA else None)


def reference(oracle, name):
    """The oracle's side of a row of PART1, computed once: the traced steps of replica 0 with the gate analysis, and the end of every
    replica's fused run.  `gated`: the steps that showed a gated multi-swap the acceptor alone would have accepted; `worse`: the steps
    that showed an accepted worsening candidate; `consumed`: candidates per step."""
    if name in _memo:
        return _memo[name]
    c = PART1[name]
    p = _problem(c["shop"], c["start"])
    args = (c["union"], c["seed"], c["acceptor"], c["param"], c["forager"], c["limit"])
    o = _oracle_shop(oracle, p, *args)
    mirror = _mirror_of(oracle, c, c["seed"])
    o.phase_start()
    cur = _score(o.score())
    mirror.phase_started(cur)
    steps, gated, worse, n_gated = [], [], [], 0
    for step in range(c["steps"]):
        om, os_, of, oap, omv = o.step_traced()
        for kind, row, fl in zip(om["kind"], os_, of):
            if not fl & 1:
                continue
            sc = _score(row)
            if fl & GATED:
                assert int(kind) == MULTI_SWAP and not sc > cur and not fl & 2
                n_gated += 1
                if step not in gated and mirror.would_accept(cur, sc):
                    gated.append(step)
            else:
                accepted = mirror.is_accepted(cur, sc)
                assert accepted == bool(fl & 2), (name, step, cur, sc)  # the restatement is the oracle's acceptor
                if accepted and sc < cur and step not in worse:
                    worse.append(step)
        cur = _score(o.score())
        mirror.step_ended(cur)
        st = o.stats()
        steps.append(dict(moves=_t(om), scores=os_[:, :2].copy(), flags=of.copy(), applied=oap, move=tuple(omv), lists=o.get_lists(0), score=cur,
                          counters=[st[k] for k in COUNTERS], anneal=_anneal_words(o) if c["acceptor"] == SA else None))
    ends = []
    for r in range(R):
        orun = _oracle_shop(oracle, p, c["union"], c["seed"] + r, *args[2:])
        orun.phase_start()
        orun.steps(c["steps"] + FUSED_EXTRA)
        assert (orun.fresh_score() == orun.score()).all()
        ends.append(_end_of(orun, c))
    _memo[name] = dict(steps=steps, gated=gated, worse=worse, n_gated=n_gated, consumed=[len(s["flags"]) for s in steps], ends=ends)
    return _memo[name]


def _device_end(d, c, r):
    st = d.stats(r)
    anneal = None
    if c["acceptor"] == SA:
        t, calibrating = d.annealing_state(r)
        anneal = (t.view(np.uint64).tolist(), calibrating)
    return (_score(d.calculate_score()[r]), _score(d.best_scores()[r]), d.working_lists(0, r), [st[k] for k in COUNTERS], anneal)


def sa_gate_is_followed_by_draws(ref):
    """The SA condition: a gated candidate that a favourable draw would have accepted, at least five further steps, an accepted worsening
    move among them (a shifted draw stream has somewhere to show)."""
    return any(len(ref["steps"]) - 1 - g >= 5 and any(w > g for w in ref["worse"]) for g in ref["gated"])


# acceptor -> the row that shows a gated multi-swap the acceptor alone would have accepted (the cheapest of those that do; picked on the
# oracle: LateAcceptance at steps 1, 2, 3, 7, 9 of its row; SimulatedAnnealing at steps 3 and 5 of 16, with accepted worsening moves at
# steps 5, 8 and 15 behind the first; DiversifiedLateAcceptance at steps 1 and 3 to 8).  Most other rows with the leaf show one as well:
# every row prints its steps.
GATE_WITNESS = {LA: "la_control", SA: "sa_ac1", DLA: "dla1_ac7"}


def test_the_table_is_the_docstrings():
    _table_is_complete()


@pytest.mark.parametrize("acceptor", list(GATE_WITNESS))
def test_the_gate_binds_where_the_acceptor_alone_would_accept(oracle, acceptor):
    """Reference side only.  HillClimbing has no such row: it accepts `sc > cur` alone, which is the gate's own condition."""
    name = GATE_WITNESS[acceptor]
    assert PART1[name]["acceptor"] == acceptor and "precedence" in UNIONS[PART1[name]["union"]][0]
    ref = reference(oracle, name)
    assert ref["gated"], name
    if acceptor == SA:
        assert sa_gate_is_followed_by_draws(ref), (ref["gated"], ref["worse"])


def _row_conditions(name, c, ref):
    print(name, "gated multi-swaps:", ref["n_gated"], "-- the acceptor alone would have accepted one at steps", ref["gated"], "-- candidates per step",
          ref["consumed"])
    if "precedence" in UNIONS[c["union"]][0] and c["start"] != "cyclic":  # (a cyclic state gives the leaf no blocks: analysis.rs:61-70)
        assert ref["n_gated"] > 0, name  # the gate turned candidates away in every run whose leaf streams
    if (c["forager"], c["limit"]) == (AC, 70):
        assert max(ref["consumed"]) > 64, name  # a step past one 64-lane replay chunk


@pytest.mark.parametrize("name", list(PART1))
def test_acceptors_the_oracle_runs(oracle, monkeypatch, name):
    c = PART1[name]
    ref = reference(oracle, name)
    _row_conditions(name, c, ref)
    mode = _place(monkeypatch, c["placement"])
    p = _problem(c["shop"], c["start"])
    args = (p, c["union"], c["seed"], c["acceptor"], c["param"], c["forager"], c["limit"])
    d = _device_shop(*args)
    d.calculate_score()
    d.phase_start()
    for step, want in enumerate(ref["steps"]):
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 18)
        assert len(gm) == len(want["moves"]), (step, len(gm), len(want["moves"]))
        assert (_t(gm) == want["moves"]).all(), step
        doable = (want["flags"] & 1) != 0
        assert (gf == want["flags"]).all() and (gs[doable] == want["scores"][doable]).all(), step
        assert gap == want["applied"] and (not gap or tuple(gmv) == want["move"]), step
        assert d.working_lists(0, 0) == want["lists"] and _score(d.calculate_score()[0]) == want["score"], step
        st = d.stats(0)
        assert [st[k] for k in COUNTERS] == want["counters"], step
        if c["acceptor"] == SA:
            t, calibrating = d.annealing_state(0)
            assert (t.view(np.uint64).tolist(), calibrating) == want["anneal"], step
    _check_placement(d, mode, p, c["union"])
    d.close()
    n = c["steps"] + FUSED_EXTRA
    for budgeted in (False, True):
        d = _device_shop(*args)
        d.calculate_score()
        d.phase_start()
        if budgeted:
            d.solve_moves(n, 1 << 30)  # no replica reaches the budget: every one runs n steps
        else:
            d.solve_steps(n // 2)
            _check_placement(d, mode, p, c["union"])
            d.solve_steps(n - n // 2)
        _check_placement(d, mode, p, c["union"])
        for r in range(R):
            assert _device_end(d, c, r) == ref["ends"][r], (budgeted, r)
        assert (d.fresh_score() == d.calculate_score()).all()
        d.close()  # (for the `plain` union _check_placement asserted prec_sweep)


# the mixed job shop (two planning classes, BendableScore<2,1>: the four-level kernels) with the critical-path leaf beside the scalar pair
MIXED_LEAVES = ("precedence", "permute", "list_change", "list_swap", "change", "swap")
MIXED = {"sa": (SA, T_EXPLICIT3, "lds_one_trial"), "dla": (DLA, 0.01, "hbm")}
MIXED_SEED, MIXED_STEPS, MIXED_LIMIT = 2, 12, 7


@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_job_shop_with_the_leaf(oracle, monkeypatch, name):
    """Part 1's comparison on the 6 x 4 mixed job shop with durations, from its acyclic start (the leaf streams): traced steps of replica 0,
    then three replicas fused both ways.  Reference side: gated multi-swaps and accepted worsening candidates occur."""
    import solverforge_amd as sfa

    acceptor, param, placement = MIXED[name]
    mode = _place(monkeypatch, placement)
    p = _mixed_problem(cyclic=False)
    c = dict(acceptor=acceptor)

    def device():
        d = sfa.build_jobshop(p, n_replicas=R, leaves=MIXED_LEAVES, makespan=True)
        d.configure(sfa.SolverConfig(acceptor=acceptor, late_acceptance_size=LA_SIZE, forager=AC, accepted_count_limit=MIXED_LIMIT, random_seed=MIXED_SEED))
        if acceptor == SA:
            d.configure_annealing(mode=param["mode"], temperatures=param["temperatures"], decay_rate=param["decay_rate"], seed=MIXED_SEED)
        else:
            d.configure_diversified(param)
        d.calculate_score()
        d.phase_start()
        return d

    def model(seed):
        o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=True, durations=p["durations"])
        o.configure(acceptor=1, la_size=LA_SIZE, forager=AC, limit=MIXED_LIMIT, leaves=sum(BITS[x] for x in MIXED_LEAVES[:4]) | 1 | 2, random_seed=seed)
        if acceptor == SA:
            o.configure_annealing(levels=3, hard_levels=2, seed=seed, **param)
        else:
            o.configure_diversified(LA_SIZE, param)
        o.phase_start()
        return o

    def placed(d):
        _assert_placement(d, mode, _mixed_as_shop(p), tables=True, owner=False, ruin_inst=False, levels=4)

    def end_of(o):
        st, anneal = o.stats(), None
        if acceptor == SA:
            t, _, calibrating = o.annealing_state()
            anneal = (t[:3].view(np.uint64).tolist(), bool(calibrating))
        return (_score(o.score(), 3), _score(o.best_score(), 3), o.get_lists(1), o.get_vars(0, 0).tolist(), [st[k] for k in COUNTERS], anneal)

    def device_end(d, r):
        st = d.stats(r)
        anneal = None
        if acceptor == SA:
            t, calibrating = d.annealing_state(r)
            anneal = (t.view(np.uint64).tolist(), calibrating)
        return (_score(d.calculate_score()[r], 3), _score(d.best_scores()[r], 3), d.working_lists(1, r), d.working_values(0, 0, replica=r).tolist(),
                [st[k] for k in COUNTERS], anneal)

    d, o = device(), model(MIXED_SEED)
    gated = worse = 0
    for step in range(MIXED_STEPS):
        cur = _score(o.score(), 3)
        om, os_, of, oap, omv = o.step_traced()
        gated += int(((of & GATED) != 0).sum())
        worse += sum(1 for row, fl in zip(os_, of) if fl & 2 and _score(row, 3) < cur)
        gm, gs, gf, gap, gmv = d.solve_step_traced(cap=1 << 16)
        assert len(gm) == len(om) and (_t(gm) == _t(om)).all() and (gf == of).all(), step
        doable = (of & 1) != 0
        assert (gs[doable] == os_[doable][:, :3]).all() and gap == oap and (not gap or tuple(gmv) == tuple(omv)), step
        assert device_end(d, 0) == end_of(o), step
    assert gated > 0 and worse > 0, (gated, worse)
    placed(d)
    n = MIXED_STEPS + FUSED_EXTRA
    ends = []
    for r in range(R):
        o = model(MIXED_SEED + r)
        o.steps(n)
        ends.append(end_of(o))
    for budgeted in (False, True):
        d = device()
        if budgeted:
            d.solve_moves(n, 1 << 30)
        else:
            d.solve_steps(n // 2)
            d.solve_steps(n - n // 2)
        placed(d)
        assert [device_end(d, r) for r in range(R)] == ends, budgeted
        assert (d.fresh_score() == d.calculate_score()).all()


# ---- part 2: GreatDeluge and StepCountingHillClimbing -----------------------------------------------------------------------------------------
P2_SHOP, P2_UNION, P2_SEED, P2_STEPS = ("6x4", "shuffled"), "four", 7, 24
# (acceptor, parameter, forager, accepted_count_limit, placement, seed): test_gpu_acceptors.TRACE on the shop.  The soft level is minus the
# makespan (some tens), so a rain speed of a few hundredths raises the water by a unit or two per step.
P2_TRACE = {"gd_first": (GD, 0.04, FA, 0, "lds", 6), "sc_first": (SC, 3, FA, 0, "hbm", 6), "sc_best": (SC, 3, BS, 0, "lds_one_trial", 6)}
P2_EQUIV_PLACEMENT = {"sc0_is_hc": "lds", "gd0_is_la": "hbm"}


def consult(record, sc, cur):
    """Does a doable candidate of a precedence model reach the acceptor?  Not a multi-swap that does not beat the last step score."""
    return not (int(record["kind"]) == MULTI_SWAP and sc <= cur)


def _p2_device(acceptor, param, forager, limit, seed, la=ta.LA_BIG):
    p = _problem(*P2_SHOP)
    d = _device_shop(p, P2_UNION, seed, n_replicas=R)
    ta._configure(d, acceptor, param, forager, limit, ta.ORDER_RANDOM, seed, la_size=la)
    return d, p


def _p2_oracle_run(oracle, acceptor, forager, limit):
    key = ("p2", acceptor, forager, limit)
    if key not in _memo:
        p, out = _problem(*P2_SHOP), []
        for r in range(R):
            o = _oracle_shop(oracle, p, P2_UNION, P2_SEED + r, acceptor=acceptor, forager=forager, limit=limit, la=ta.LA_BIG)
            o.phase_start()
            o.steps(P2_STEPS)
            st = o.stats()
            out.append((list(_score(o.score())), list(_score(o.best_score())), o.get_lists(0), [st[k] for k in COUNTERS]))
        _memo[key] = out
    return _memo[key]


@pytest.mark.parametrize("which", list(ta.EQUIV))
def test_equivalences_on_the_precedence_union(oracle, monkeypatch, which):
    """StepCounting(limit 0) is HillClimbing; GreatDeluge(rain speed 0) is LateAcceptance with a history longer than the run -- with the
    gate in front of either."""
    acceptor, param, o_acceptor, forager, limit = ta.EQUIV[which]
    want = _p2_oracle_run(oracle, o_acceptor, forager, limit)
    if which == "gd0_is_la":
        assert ta._differ(want, _p2_oracle_run(oracle, HC, forager, limit), 2)
    mode = _place(monkeypatch, P2_EQUIV_PLACEMENT[which])
    d, p = _p2_device(acceptor, param, forager, limit, P2_SEED)
    d.solve_steps(P2_STEPS // 2)
    d.solve_steps(P2_STEPS - P2_STEPS // 2)
    _check_placement(d, mode, p, P2_UNION)
    for r, (got, exp) in enumerate(zip(ta._snapshot(d, "prec", True), want)):
        assert got[:4] == tuple(exp), (r, got[:2], exp[:2])


def _p2_traced(oracle, run, replica=0):
    """(events, snapshot of all replicas) of a traced run -- the environment of the run's placement is the caller's."""
    key = ("p2_traced", run, replica)
    if key not in _memo:
        acceptor, param, forager, limit, mode, seed = P2_TRACE[run]
        d, p = _p2_device(acceptor, param, forager, limit, seed)
        o = _oracle_shop(oracle, p, P2_UNION, seed + replica)
        events = ta.trace_replica(oracle, d, "prec", acceptor, param, replica, P2_STEPS, o=o, consult=consult)
        _check_placement(d, mode, p, P2_UNION)
        _memo[key] = (dict(events), ta._snapshot(d, "prec", True))
        d.close()
    return _memo[key]


@pytest.mark.parametrize("replica", [0, 2])
@pytest.mark.parametrize("run", list(P2_TRACE))
def test_great_deluge_and_step_counting_traced(oracle, monkeypatch, run, replica):
    _place(monkeypatch, P2_TRACE[run][4])
    events, snap = _p2_traced(oracle, run, replica)
    print(run, replica, "events -> first step:", events)
    assert "gate_alone_refused" in events, sorted(events)  # the gate bound where the water level / the open door alone would have accepted
    if run == "gd_first":
        assert {"accepted_through_water_only", "refused_below_water"} <= set(events), sorted(events)
    if run == "sc_first":
        assert {"since_reached_limit", "since_reset_afterwards"} <= set(events), sorted(events)
    if replica:
        assert snap == _p2_traced(oracle, run, 0)[1]  # the launch moves every replica whichever one is traced
    assert len({str(s[2]) for s in snap}) == R


def test_great_deluge_and_step_counting_events(oracle, monkeypatch):
    seen = set()
    for run in P2_TRACE:
        with monkeypatch.context() as m:
            _place(m, P2_TRACE[run][4])
            seen |= set(_p2_traced(oracle, run)[0])
    assert not [e for e in ta.EVENTS if e not in seen], sorted(seen)


@pytest.mark.parametrize("run", list(P2_TRACE))
def test_great_deluge_and_step_counting_fused(oracle, monkeypatch, run):
    acceptor, param, forager, limit, mode, seed = P2_TRACE[run]
    _place(monkeypatch, mode)
    want = _p2_traced(oracle, run)[1]
    for budgeted in (False, True):
        d, p = _p2_device(acceptor, param, forager, limit, seed)
        if budgeted:
            d.solve_moves(P2_STEPS, 1 << 30)
        else:
            d.solve_steps(P2_STEPS // 2)
            d.solve_steps(P2_STEPS - P2_STEPS // 2)
        _check_placement(d, mode, p, P2_UNION)
        assert ta._snapshot(d, "prec", True) == want, budgeted


# ---- part 3: TabuSearch -----------------------------------------------------------------------------------------------------------------------
P3_STEPS = 30
# site -> (policy [entity, value, move, undo, aspiration], forager, accepted_count_limit, placement)
P3 = {"shop": ([3, 3, 6, 6, True], AC, 70, "hbm"), "mixed": ([3, 3, 6, 6, True], BS, 0, "lds")}


def _mixed_problem(cyclic=True):
    """The 6 x 4 mixed job shop with durations (tests/test_gpu_precedence.py: test_mixed_jobshop_with_makespan's construction)."""
    from solverforge_amd import datasets

    p = datasets.construct_jobshop(datasets.make_jobshop(6, 4), seed=3)
    p["durations"] = (datasets.stream(5, p["n_ops"]) % np.uint64(9)).astype(np.int64) + 1
    if cyclic:
        p["sequences"][2] = p["sequences"][2][::-1]  # one machine against the job order: cycles
    return p


def _mixed_as_shop(p):
    """What _assert_placement reads of a precedence shop, for the mixed model: the job order as fixed successors."""
    n, job = p["n_ops"], np.asarray(p["job"])
    successors = [[op + 1] if op + 1 < n and job[op + 1] == job[op] else [] for op in range(n)]
    return {"durations": p["durations"], "sequences": p["sequences"], "successors": successors}


def _p3_pair(oracle, site):
    import solverforge_amd as sfa

    if site == "shop":
        p = _problem("6x4", "shuffled")
        d = sfa.build_precedence_shop(p, n_replicas=R, leaves=UNIONS["plain"][0])
        o = oracle.Model.precedence_shop(p["durations"], p["successors"], p["sequences"], p["expected_owner"])
        return d, o, p, "generic", None, lambda dd, mode: _check_placement(dd, mode, p, "plain")
    p = _mixed_problem()
    d = sfa.build_jobshop(p, n_replicas=R, makespan=True)
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=True, durations=p["durations"])
    packer = tm.ModelPacker({tt.SCALAR_SCOPE["mixed"]: (0, 0, 0), tt.LIST_SCOPE["mixed"]: (1, p["n_ops"], p["n_machines"] + 1)})
    return d, o, p, "mixed", packer, lambda dd, mode: _assert_placement(dd, mode, _mixed_as_shop(p), tables=False, owner=False, ruin_inst=False, levels=4)


def _p3_traced(oracle, site, replica=0):
    key = ("p3", site, replica)
    if key not in _memo:
        policy, forager, limit, mode = P3[site]
        d, o, p, tsite, packer, placed = _p3_pair(oracle, site)
        tt._configure(d, policy, forager, limit)
        events = tt.trace_replica(oracle, d, tsite, policy, replica, P3_STEPS, o=o, packer=packer)
        placed(d, mode)
        _memo[key] = (dict(events), tt._snapshot(d, tsite))
        d.close()
    return _memo[key]


@pytest.mark.parametrize("replica", [0, 2])
@pytest.mark.parametrize("site", list(P3))
def test_tabu_search_traced(oracle, monkeypatch, site, replica):
    _place(monkeypatch, P3[site][3])
    events, snap = _p3_traced(oracle, site, replica)
    print(site, replica, "events -> first step:", events)
    for memory, tenure in zip(tm.MEMORIES, P3[site][0][:4]):
        if tenure is not None:
            assert "refused_with_%s" % memory in events, (memory, sorted(events))
    assert "admissible_again_after_eviction" in events, sorted(events)
    if replica:
        assert snap == _p3_traced(oracle, site, 0)[1]
    assert len({str(s[2]) for s in snap}) == R


@pytest.mark.parametrize("site", list(P3))
def test_tabu_search_fused(oracle, monkeypatch, site):
    policy, forager, limit, mode = P3[site]
    _place(monkeypatch, mode)
    want = _p3_traced(oracle, site)[1]
    for budgeted in (False, True):
        d, o, p, tsite, packer, placed = _p3_pair(oracle, site)
        tt._configure(d, policy, forager, limit)
        for n in (P3_STEPS // 2, P3_STEPS - P3_STEPS // 2):
            if budgeted:
                d.solve_moves(n, 1 << 30)
            else:
                d.solve_steps(n)
            placed(d, mode)
        assert tt._snapshot(d, tsite) == want, budgeted


def test_tabu_search_refuses_the_critical_path_leaf():
    import solverforge_amd as sfa

    d = sfa.build_precedence_shop(_problem("6x4", "scheduled"), n_replicas=2, leaves=("precedence", "list_change", "list_swap"))
    tt._configure(d, [2, None, 5, None, True], AC, 7)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED.*tabu search.*variable-length"):
        d.solve_steps(2)


# ---- part 4: Variable Neighborhood Descent and LimitedNeighborhood ---------------------------------------------------------------------------
P4_SEED = 9
PLAIN_BITS = [BITS[x] for x in UNIONS["plain"][0]]


def test_vnd_to_its_end(oracle, monkeypatch):
    """The two plain list leaves as two neighbourhoods, from the shuffled start, every replica to its end; replica 1 is traced against the
    mirror.  At the end no neighbourhood holds a strictly improving candidate by the oracle's enumerate / evaluate_moves."""
    mode = _place(monkeypatch, "hbm")
    p = _problem("6x4", "shuffled")
    r = 1
    d = _device_shop(p, "plain", P4_SEED)
    d.configure_vnd()
    d.calculate_score()
    d.phase_start()
    o = _oracle_shop(oracle, p, "plain", P4_SEED + r)
    mirror = vm.VndPhase(o, PLAIN_BITS, lambda s: oracle.lib().sfo_step_seed(P4_SEED + r, s))
    steps = 0
    while not mirror.done:
        assert d.vnd_state(r) == mirror.state(), steps
        cur = mirror.current
        gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 14)
        rec = mirror.step()
        assert len(gm) == rec["cursor"] and (_t(gm) == _t(rec["moves"])).all(), steps
        assert ((gf & 1) != 0).tolist() == rec["doable"] and ((gf >> 8) == rec["k"]).all(), steps
        assert [tuple(row) for row, ok in zip(gs.tolist(), rec["doable"]) if ok] == [sc for sc, ok in zip(rec["scores"], rec["doable"]) if ok], steps
        assert ((gf & 2) != 0).tolist() == [ok and vm.accepts(sc, cur) for sc, ok in zip(rec["scores"], rec["doable"])], steps
        assert np.flatnonzero(gf & 4).tolist() == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), steps
        assert _score(d.calculate_score()[r]) == rec["score"], steps
        steps += 1
    assert steps > len(PLAIN_BITS) and mirror.stats["moves_applied"] > 0  # a descent, not a start at an optimum
    _check_placement(d, mode, p, "plain")
    assert d.vnd_state(r) == mirror.state() and d.vnd_state(r)["done"]
    st = d.stats(r)
    assert [st[k] for k in vm.COUNTERS] == [mirror.stats[k] for k in vm.COUNTERS]
    assert d.working_lists(0, r) == o.get_lists(0)
    assert vm.is_local_optimum(o, PLAIN_BITS)
    assert d.solve_vnd(500, steps_per_launch=8) == R  # the other replicas, fused
    _check_placement(d, mode, p, "plain")
    assert (d.fresh_score() == d.calculate_score()).all()
    for q in range(R):
        oq = oracle.Model.precedence_shop(p["durations"], p["successors"], d.working_lists(0, q), p["expected_owner"])
        oq.configure(leaves=sum(PLAIN_BITS))
        assert _score(oq.score()) == _score(d.calculate_score()[q]) and vm.is_local_optimum(oq, PLAIN_BITS), q
    fused = _device_shop(p, "plain", P4_SEED)
    fused.configure_vnd()
    fused.calculate_score()
    fused.phase_start()
    assert fused.solve_vnd(500, steps_per_launch=5) == R
    for q in range(R):
        assert fused.working_lists(0, q) == d.working_lists(0, q) and fused.stats(q) == d.stats(q), q


# name -> (union order, child limits, root limit, acceptor, forager, placement)
P4_LIMITED = {"child_65_round_robin": (lm.ROUND_ROBIN, [65, None], None, HC, BS, "lds"),
              "root_64_stratified": (lm.STRATIFIED_RANDOM, [None, None], 64, LA, BS, "lds_one_trial")}
P4_STEPS = 5


@pytest.mark.parametrize("name", list(P4_LIMITED))
def test_limited_neighbourhoods(oracle, monkeypatch, name):
    order, child, root, acceptor, forager, mode = P4_LIMITED[name]
    _place(monkeypatch, mode)
    p = _problem("6x4", "shuffled")

    def device():
        d = _device_shop(p, "plain", P4_SEED, acceptor=acceptor, forager=forager, limit=3, la=5, random_ties=False)
        for leaf, lim in enumerate(child):
            d.limit_selector(leaf, lim)
        d.configure_union(order, None)
        d.limit_union(root)
        d.calculate_score()
        d.phase_start()
        return d

    ends = []
    for r in (0, 2):
        d = device()
        o = _oracle_shop(oracle, p, "plain", P4_SEED + r, random_ties=False)
        mirror = lm.LimitedSearch(oracle, o, PLAIN_BITS, P4_SEED + r, union_order=order, child_limits=child, root_limit=root, acceptor=acceptor, la_size=5,
                                  forager=forager, limit=3, order=3)
        bound = 0
        for step in range(P4_STEPS):
            gm, gs, gf, gap, gmv = d.solve_step_traced(replica=r, cap=1 << 14)
            rec = mirror.step()
            cands = rec["candidates"][:rec["consumed"]]
            assert _t(gm).tolist() == [list(c["record"]) for c in cands], (r, step)
            assert ((gf & 1) != 0).tolist() == [c["doable"] for c in cands], (r, step)
            assert [tuple(row) for row, c in zip(gs.tolist(), cands) if c["doable"]] == [c["score"] for c in cands if c["doable"]], (r, step)
            assert ((gf & 2) != 0).tolist() == rec["accepted"] and (gf >> 8).tolist() == [c["child"] for c in cands], (r, step)
            assert np.flatnonzero(gf & 4).tolist() == ([] if rec["pick"] is None else [rec["pick"]]) and gap == (rec["pick"] is not None), (r, step)
            assert _score(d.calculate_score()[r]) == rec["score"], (r, step)
            st = d.stats(r)
            assert [st[k] for k in lm.COUNTERS] == [mirror.stats[k] for k in lm.COUNTERS], (r, step)
            if root is not None:
                bound += rec["consumed"] == root < sum(rec["lengths"])
            else:
                bound += [c["child"] for c in cands].count(0) == child[0] < rec["lengths"][0]
        assert bound == P4_STEPS  # the limit cut every step's cursor short
        _check_placement(d, mode, p, "plain")
        assert d.working_lists(0, r) == o.get_lists(0)
        ends.append([(d.working_lists(0, q), d.stats(q)) for q in range(R)])
    assert ends[0] == ends[1]
    fused = device()
    fused.solve_steps(2)
    fused.solve_steps(P4_STEPS - 2)
    _check_placement(fused, mode, p, "plain")
    assert [(fused.working_lists(0, q), fused.stats(q)) for q in range(R)] == ends[0]
    assert (fused.fresh_score() == fused.calculate_score()).all()


# ---- part 5: MODE 2 ---------------------------------------------------------------------------------------------------------------------------
P5_R, P5_STEPS = 2049, 6
P5_SAMPLE = (0, 1, 63, 64, 255, 256, 511, 777, 1023, 1024, 1500, 1501, 2046, 2047, 2048, 1999)
P5 = {"hc": (HC, None, AC, 7, 51), "sa": (SA, T_EXPLICIT, AC, 7, 52), "dla": (DLA, 0.01, AC, 7, 53)}


@pytest.mark.parametrize("name", list(P5))
def test_mode2_under_other_acceptors(oracle, monkeypatch, name):
    """2,049 replicas with the grouped evaluator off take the PREC build for four workgroups per CU (prec_occ, asserted); untraced, six
    fused steps; sixteen replicas -- the first, both sides of 2,048, the last -- against an oracle model of their own."""
    acceptor, param, forager, limit, seed = P5[name]
    assert len(set(P5_SAMPLE)) == 16 and {0, 2047, 2048} <= set(P5_SAMPLE) and max(P5_SAMPLE) == P5_R - 1
    _place(monkeypatch, "lds_one_trial")
    p = _problem("6x4", "scheduled")
    c = dict(acceptor=acceptor)
    d = _device_shop(p, "four", seed, acceptor, param, forager, limit, n_replicas=P5_R)
    d.calculate_score()
    d.phase_start()
    d.solve_steps(P5_STEPS)
    _assert_placement(d, "lds_one_trial", p, prec_occ=True, ruin_inst=False)
    scores = d.calculate_score()
    assert (d.fresh_score() == scores).all()
    for r in P5_SAMPLE:
        o = _oracle_shop(oracle, p, "four", seed + r, acceptor, param, forager, limit)
        o.phase_start()
        o.steps(P5_STEPS)
        assert _device_end(d, c, r) == _end_of(o, c), r
