"""GPU parity tests (through the C ABI) on both sides of every gate by which the host places a precedence (job-shop makespan) model's
fused launch (csrc/sf_mixed_plan.h: plan_generic_launch).  Every case builds a model on one side of one gate, runs a fused launch,
asserts the placement the library recorded (sf_list_arith_flags -> GpuScoreDirector.arith_flags: PREC instantiation, Kahn scratch in
LDS, static copy none / full / slim, grouped trials T, MODE 2, sweep, incremental refresh, RUIN instantiation, level template, value
bytes), then compares with the CPU oracle in integer equality: full score, fresh score and evaluate_each of a scheduled, a reversed
(cyclic) and a partly assigned state; the trial scores of a whole cursor over the six list move kinds where the graph is small
(under 100 nodes -- from 200 nodes on the oracle's cursor costs more than every other case of this file together); a fused window
(lists, scores, best score, five counters, fresh_score == calculate_score).

Edge sizes, from the host's own formulas (n nodes, E valid fixed edges, V lists; all integer):
  Kahn scratch        prec_lds_scratch_bytes = 12 n.  <= 36 KiB (n <= 3,072): LDS.  Above: LDS while GCarve<int16_t>(...).total + 1,024
                      <= SF_LDS_BUDGET = 162,816, else HBM with the lane-per-trial sweep.  SF_AMD_PREC_LDS_MAX_KB=36 caps it at 3,072 nodes.
                      For a list-only model of 8 lists the carve is 14 n + 8 V + 4 (V + 1) + 768 rounded per array to 16 bytes:
                      n = 11,493 -> 161,792 (in), n = 11,494 -> 161,808 (+ 1,024 = 162,832: out).
  full static copy    prec_static_bytes = 4 (n (owner ? 3 : 2) + 2 (n + 1) + 2 E + 2 n) + 16 = (owner ? 28 : 24) n + 8 E + 24 <= 16,384:
                      owners n = 500: E = 295 in (16,384), 296 out; no owners n = 600: E = 245 in (16,384), 246 out.
  slim static copy    prec_static_slim_bytes = (owner ? 16 : 12) n + 16 <= 40,960: owners 2,559 in / 2,560 out; none 3,412 in / 3,413 out.
  cv2 fit             the copy is dropped when slice + 1,024 + copy > 162,816: 3,400 nodes without owners (copy 40,816) on 8 lists with an
                      element capacity of 39,648 (slice 120,976: in, sum 162,816) / 39,649 (out).
  groups' fit         the plan repeats that test on the slice WITH the grouped evaluator's scratch and halves T until it passes:
                      428 nodes, 5 lists (T = 2, scratch 14,304; copy 13,720): capacity 63,888 in (162,808), 63,889 out (T = 0);
                      SF_AMD_PREC_GROUPS=16 on 300 nodes, 3 lists: 57,928 keeps 8 / 57,929 -> 4; 65,160 keeps 4 / 65,161 -> 2.
  grouped evaluator   needs the full copy.  g = largest power of two <= max(V, 2), t = min(16, 64 / g), halved while
                      b = pgrp_bytes(n, t, V) > 14,336 and b + 16 n + 2,560 > 20,480; V >= 64: off.
                      pgrp_bytes = 4 a2 + a16(4 V) + t (2 a16(4 (n + 64 / t)) + 2 a2), a2 = a16(2 n), a16 = round up to 16.
                      V = 5: n = 80 -> T 16 by the second rule (b = 16,544, sum 20,384), 81 -> 8 (17,632 / 21,488);
                      n = 244 -> T 4 by the first rule (b = 14,304), 245 -> 2 (14,432, sum 20,912); n = 428 -> 2 (14,304), 429 -> 0 (14,368).
  MODE 2              untraced, T = 0, replicas > 2,048, 163,840 / (slice + 256) > 8 <=> slice <= 17,948.  30 x 20 shop: 9,424;
                      50 x 20 nine-leaf: 16,080; 8 lists, two leaves: n = 1,217 -> 17,936 (in), 1,218 -> 17,952 (out).
  one-byte values     n_values <= 127 and >= 1,024 scalar entities, in the L = 2 and the L = 4 template.
The carve totals were computed with the host's GCarve on the host, and test_generic_plan.py asserts them there (no GPU); the asserted
placements fail loudly if the carve changes.

The host-driven entry points (sf_evaluate_all, sf_step_evaluate, sf_apply) read none of the SF_AMD_PREC_* variables: their Kahn scratch is
the model's HBM arrays always (one wavefront per replica / record, list copies in LDS), so there is no placement to record for them."""
import numpy as np
import pytest
from prec_placement_rules import default_trials, pgrp_bytes  # (tests/: the host's rules restated once)

pytestmark = pytest.mark.gpu

LEAF_BITS = {"precedence": 16384, "permute": 8192, "list_change": 4, "list_swap": 8, "list_reverse": 64, "sublist_change": 128,
             "sublist_swap": 256, "kopt": 512, "ruin": 1024}
SIX = ("list_change", "list_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt")
NINE = ("precedence", "permute", "list_change", "list_swap", "sublist_change", "sublist_swap", "list_reverse", "kopt", "ruin")
COUNTERS = ["step_count", "moves_evaluated", "moves_accepted", "moves_applied", "score_calculations"]
PREC_VARS = ("SF_AMD_PREC_HBM", "SF_AMD_PREC_INC", "SF_AMD_PREC_NO_SWEEP", "SF_AMD_PREC_GROUPS", "SF_AMD_PREC_STATIC_HBM", "SF_AMD_PREC_STATIC_SLIM",
             "SF_AMD_PREC_LDS_MAX_KB", "SF_AMD_PLF_SLOW", "SF_AMD_PLF_FORCE64")


@pytest.fixture(autouse=True)
def default_settings(monkeypatch):
    for k in PREC_VARS:
        monkeypatch.delenv(k, raising=False)


def _t(moves):
    return np.stack([moves["kind"], moves["a"], moves["a_pos"], moves["b"], moves["b_pos"], moves["value"]], axis=1)


def test_formulas_at_the_documented_edges():
    """The sizes in the module docstring sit where it says they do (host arithmetic only; the GPU cases assert what the library did)."""
    assert 28 * 500 + 8 * 295 + 24 == 16384 and 24 * 600 + 8 * 245 + 24 == 16384
    assert 16 * 2559 + 16 <= 40960 < 16 * 2560 + 16 and 12 * 3412 + 16 == 40960
    assert 12 * 3072 == 36 * 1024
    assert [default_trials(n, 5) for n in (80, 81, 244, 245, 428, 429)] == [16, 8, 4, 2, 2, 0]
    assert pgrp_bytes(80, 16, 5) > 14336 and pgrp_bytes(80, 16, 5) + 16 * 80 + 2560 <= 20480 < pgrp_bytes(81, 16, 5) + 16 * 81 + 2560
    assert pgrp_bytes(244, 4, 5) <= 14336 < pgrp_bytes(245, 4, 5) and pgrp_bytes(245, 4, 5) + 16 * 245 + 2560 > 20480
    assert pgrp_bytes(428, 2, 5) <= 14336 < pgrp_bytes(429, 2, 5)
    assert 163840 // (17936 + 256) == 9 and 163840 // (17952 + 256) == 8
    assert 120976 + 1024 + 12 * 3400 + 16 == 162816


def _graph(n, E, V, seed=1, empty_last=False):
    """A general precedence graph: fixed edges k -> k + 1 for k < E (E <= n - 1), durations 1..9 from the documented stream, the expected
    owner of node v = v % (lists in use) except that every third node belongs to list 0 (lists of unequal length; empty_last keeps the
    last list empty).  Scheduled state: every list holds its nodes in ascending order (all edges point forward: acyclic)."""
    from solverforge_amd import datasets

    assert E <= n - 1
    used = max(1, V - 1) if empty_last else V
    succ = [[v + 1] if v < E else [] for v in range(n)]
    dur = (datasets.stream(seed + 31, n) % np.uint64(9)).astype(np.int64) + 1
    owner = np.array([0 if v % 3 == 0 else v % used for v in range(n)], dtype=np.int64)
    seqs = [[] for _ in range(V)]
    for v in range(n):
        seqs[int(owner[v])].append(v)
    return {"durations": dur, "successors": succ, "expected_owner": owner, "sequences": seqs}


def _states(p):
    """scheduled, reversed (every list back to front: the fixed chain closes cycles through the lists), partly assigned (every fifth node
    in no list, the lists reversed pairwise)."""
    rev = dict(p, sequences=[list(reversed(s)) for s in p["sequences"]])
    part = dict(p, sequences=[[x for x in (s if i % 2 else reversed(s)) if x % 5 != 2] for i, s in enumerate(p["sequences"])])
    return [("scheduled", p), ("reversed", rev), ("partly", part)]


def _pair(oracle, p, leaves, owner=True, R=1, seed=6, la=5, limit=12, levels=2, policy=False, ruin=(2, 4, 3), capacity=None, forager=0):
    import solverforge_amd as sfa

    kw = dict(levels=3, hard_levels=2, hard_level=1, makespan_level=2) if levels == 3 else {}
    okw = dict(levels=3, hard_levels=2, hard_level=1, soft_level=2) if levels == 3 else {}
    d = sfa.build_precedence_shop(p, n_replicas=R, leaves=leaves, with_owner=owner, ruin=ruin, precedence_policy=policy, element_capacity=capacity, **kw)
    d.configure(sfa.SolverConfig(random_seed=seed, late_acceptance_size=la, accepted_count_limit=limit, forager=forager))
    bits = sum(LEAF_BITS[x] for x in leaves)

    def mk(s, order=3):
        o = oracle.Model.precedence_shop(p["durations"], p["successors"], p["sequences"], p["expected_owner"] if owner else None, **okw)
        o.configure(leaves=bits, random_seed=s, la_size=la, limit=limit, selection_order=order, forager=forager)
        if "ruin" in leaves:
            o.set_ruin(ruin[0], ruin[1], ruin[2])
        if "kopt" in leaves:
            o.set_kopt(1, 0)
        o.set_precedence_policy(policy)
        return o

    return d, mk


def _placed(d, want):
    """The recorded placement of the last fused launch holds every field of `want`."""
    gen = d.arith_flags()[1]
    assert gen is not None and gen["prec"], gen
    got = {k: gen[k] for k in want}
    assert got == want, (got, want, gen)


def _full_scores(oracle, p, owner, levels=2):
    """Full score, fresh score and evaluate_each of the three states; the reversed one must be cyclic (hard penalty)."""
    L = levels
    for name, q in _states(p):
        d, mk = _pair(oracle, q, ("list_change", "list_swap"), owner=owner, levels=levels)
        o = mk(1)
        want = o.score()[:L]
        assert (d.calculate_score()[0] == want).all(), (name, want)
        assert (d.fresh_score()[0] == want).all(), name
        gs, gc = d.evaluate_each()
        os_, oc = o.evaluate_each()
        assert (gs == os_[:, :L]).all() and (gc == oc).all(), name
        if name == "reversed":
            assert want[levels - 2] < 0, want


def _cursor(oracle, p, owner, want):
    """Trial scores of a whole cursor over the six list move kinds (a traced fused launch), scheduled and reversed state."""
    for name, q in _states(p)[:2]:
        d, mk = _pair(oracle, q, SIX, owner=owner)
        d.calculate_score()
        for order in (0, 3):
            o = mk(1, order)
            gm, gs, gd = d.open_cursor(2, 31, selection_order=order, cap=1 << 20)
            om = o.enumerate(0, 2, 31, order)
            assert len(gm) == len(om) > 0 and (_t(gm) == _t(om)).all(), (name, order)
            os_, od = o.evaluate_moves(om)
            assert (gd == od).all() and (gs == os_[:, :2]).all(), (name, order)
        _placed(d, dict(want, prec_occ=False))


def _window(oracle, p, want, leaves=("list_change", "list_swap", "sublist_change", "list_reverse"), owner=True, R=1, replicas=(0,), steps=4, seed=6,
            levels=2, **kw):
    """A fused window of `steps` steps on R replicas: the placement, then lists, scores, best score and the five counters of the named
    replicas against their own oracle runs, and fresh_score == calculate_score over all replicas."""
    L = levels
    d, mk = _pair(oracle, p, leaves, owner=owner, R=R, seed=seed, levels=levels, **kw)
    d.calculate_score()
    d.phase_start()
    d.solve_steps(steps)
    _placed(d, want)
    scores = d.calculate_score()
    best = d.best_scores()
    for r in replicas:
        o = mk(seed + r)
        o.phase_start()
        o.steps(steps)
        assert d.working_lists(0, r) == o.get_lists(0), r
        assert (scores[r] == o.score()[:L]).all(), (r, scores[r], o.score())
        assert (best[r] == o.best_score()[:L]).all(), r
        gst, ost = d.stats(r), o.stats()
        for c in COUNTERS:
            assert gst[c] == ost[c], (r, c)
    assert (d.fresh_score() == scores).all()
    return d


LDS = dict(prec_lds=True, prec_sweep=False, prec_inc=False, ruin_inst=False, levels=2, value_bytes=2)


# ---- full static copy, 16 KiB ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner,n,E,static", [(True, 500, 295, 1), (True, 500, 296, 2), (False, 600, 245, 1), (False, 600, 246, 2)])
def test_full_static_copy_edge(oracle, owner, n, E, static):
    """The last graph whose full static copy fits 16,384 bytes and the first that takes the slim one: there the grouped evaluator is off
    (its node records live in the full copy).  12 lists: T = 8 by the list count, halved by bytes to what default_trials gives."""
    V = 12
    p = _graph(n, E, V, seed=3)
    T = default_trials(n, V) if static == 1 else 0
    assert ((28 if owner else 24) * n + 8 * E + 24 <= 16384) == (static == 1)
    _full_scores(oracle, p, owner)
    _window(oracle, p, dict(LDS, prec_static=static, prec_groups=T, prec_occ=False), owner=owner)


# ---- slim static copy, 40 KiB ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner,n,static", [(True, 2559, 2), (True, 2560, 0), (False, 3412, 2), (False, 3413, 0)])
def test_slim_static_copy_edge(oracle, owner, n, static):
    """The last graph whose slim copy fits 40,960 bytes and the first whose node records come from HBM.  (3,412 / 3,413 nodes also pass
    the whole-slice rule of the Kahn scratch: 12 n > 36 KiB.)"""
    p = _graph(n, n // 2, 8, seed=4)
    _full_scores(oracle, p, owner)
    _window(oracle, p, dict(LDS, prec_static=static, prec_groups=0, prec_occ=False), owner=owner, leaves=("list_change", "list_swap"))


# ---- grouped evaluator: tiers by list count ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,T", [(1, 16), (2, 16), (3, 16), (4, 16), (5, 16), (8, 8), (9, 8), (16, 4), (17, 4), (32, 2), (33, 2), (63, 2), (64, 0), (65, 0)])
def test_grouped_tiers_by_list_count(oracle, V, T):
    """48 nodes (every scratch size fits): T = min(16, 64 / g), g = the largest power of two <= max(V, 2); 64 lists and more: off.  Lists of
    unequal length, the last one empty (V >= 2), most of them empty at V >= 32."""
    n = 48
    p = _graph(n, 30, V, seed=V, empty_last=True)
    assert default_trials(n, V) == T
    want = dict(LDS, prec_static=1, prec_groups=T)
    _full_scores(oracle, p, True)
    _cursor(oracle, p, True, want)
    _window(oracle, p, dict(want, prec_occ=False), leaves=SIX if V > 1 else ("list_change", "list_swap", "list_reverse"), steps=12, limit=20)


# ---- grouped evaluator: tiers by bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,cursor", [(80, 16, True), (81, 8, True), (244, 4, False), (245, 2, False), (428, 2, False), (429, 0, False)])
def test_grouped_tiers_by_bytes(oracle, n, T, cursor):
    """Five lists (16 trials by the list count).  80 / 81 nodes: the 20 KiB rule (scratch + 16 n + 2,560) lets 16 trials go to 8; 244 / 245:
    the 14 KiB rule, 4 -> 2; 428 / 429: the 14 KiB rule switches the evaluator off."""
    V = 5
    p = _graph(n, n // 2, V, seed=n, empty_last=True)
    assert default_trials(n, V) == T and 28 * n + 8 * (n // 2) + 24 <= 16384
    want = dict(LDS, prec_static=1, prec_groups=T)
    _full_scores(oracle, p, True)
    if cursor:
        _cursor(oracle, p, True, want)
    _window(oracle, p, dict(want, prec_occ=False), steps=6 if n < 100 else 4)


# ---- Kahn scratch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap36,lds", [(3072, False, True), (3073, False, True), (3072, True, True), (3073, True, False)])
def test_kahn_scratch_36k_edge(oracle, monkeypatch, n, cap36, lds):
    """36,864 bytes of scratch (3,072 nodes) are the last that go to LDS unconditionally; 3,073 nodes pass the whole-slice rule and stay in
    LDS -- or, with SF_AMD_PREC_LDS_MAX_KB=36, go to HBM with the lane-per-trial sweep."""
    if cap36:
        monkeypatch.setenv("SF_AMD_PREC_LDS_MAX_KB", "36")
    p = _graph(n, n // 2, 8, seed=5)
    _full_scores(oracle, p, False)
    # (no owners: the slim copy of 12 n + 16 bytes fits)
    _window(oracle, p, dict(LDS, prec_lds=lds, prec_sweep=not lds, prec_static=2 if lds else 0, prec_groups=0, prec_occ=False), owner=False,
            leaves=("list_change", "list_swap"))


@pytest.mark.parametrize("n,lds", [(11493, True), (11494, False)])
def test_kahn_scratch_whole_slice_flip(oracle, n, lds):
    """The largest graph on 8 lists whose whole replica slice (161,792 bytes + 1,024) still fits a CU's LDS budget, and the first whose
    scratch goes to HBM (161,808 + 1,024 > 162,816).  Full scores and two fused steps."""
    p = _graph(n, n // 2, 8, seed=7)
    d, mk = _pair(oracle, p, ("list_change", "list_swap"))
    o = mk(1)
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()
    q = _states(p)[2][1]
    d, mk = _pair(oracle, q, ("list_change", "list_swap"))
    o = mk(1)
    assert (d.calculate_score()[0] == o.score()[:2]).all() and (d.fresh_score()[0] == o.score()[:2]).all()
    _window(oracle, p, dict(LDS, prec_lds=lds, prec_sweep=not lds, prec_static=0, prec_groups=0, prec_occ=False), leaves=("list_change", "list_swap"), steps=2)


# ---- the static copy beside a large slice -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,static", [(39648, 2), (39649, 0)])
def test_static_copy_dropped_when_the_slice_leaves_no_room(oracle, capacity, static):
    """3,400 nodes without owners (slim copy 40,816 bytes) on a list class of a large element capacity: slice 120,976 + 1,024 + copy =
    162,816 fits exactly at capacity 39,648; one element more and the copy stays in HBM -- the launch succeeds either way."""
    p = _graph(3400, 1700, 8, seed=8)
    _window(oracle, p, dict(LDS, prec_static=static, prec_groups=0, prec_occ=False), owner=False, leaves=("list_change", "list_swap"), capacity=capacity)


@pytest.mark.parametrize("forced,n,V,capacity,T", [(False, 428, 5, 63888, 2), (False, 428, 5, 63889, 0), (True, 300, 3, 57928, 8), (True, 300, 3, 57929, 4),
                                                   (True, 300, 3, 65160, 4), (True, 300, 3, 65161, 2)])
def test_groups_scratch_overflow_halves_the_groups(oracle, monkeypatch, forced, n, V, capacity, T):
    """The fit test of the static copy runs before the grouped evaluator is chosen, on a slice without its scratch, so the real carve can
    pass a CU's LDS where the estimate fitted.  Such a launch used to be refused (SF_ERR_UNSUPPORTED: "one replica's LDS slice ... exceeds
    a CU's 160 KiB" / "model does not fit one wave's LDS slice"); plan_generic_launch now repeats the same fit test (slice + 1,024 + copy <=
    162,816) on its own carve and halves the groups until it passes; the copy stays (without groups the slice is the one the estimate
    passed).  It is reachable under DEFAULT settings by a small graph on a list class of a large element capacity:
      428 nodes, 5 lists, 214 edges, owners: full copy 28 n + 8 E + 24 = 13,720; T = 2, scratch 14,304.  Capacity 63,888: slice without
      groups 133,760, with them 148,064, + 1,024 + 13,720 = 162,808: kept.  Capacity 63,889: 148,080 + 14,744 = 162,824 > 162,816 (the
      estimate, 133,776 + 14,744, still passes): groups off.
    and with SF_AMD_PREC_GROUPS=16:
      300 nodes, 3 lists, 150 edges: copy 9,624; 16 trials need 60,816 bytes (> 40 KiB), 8 run on 31,888, 4 on 17,424, 2 on 10,192.
      Capacity 57,928: slice 152,160, + 1,024 + 9,624 = 162,808: 8 kept.  57,929: 152,176 + 10,648 = 162,824: 4 (137,712 + 10,648).
      Capacity 65,160: 4 trials on 152,160: kept.  65,161: 152,176: 2 (144,944 + 10,648).
    (Up to the full 163,840 bytes the launch itself fails: the PREC kernels hold 1,184 bytes of static LDS, not the 1,024 the rule counts.)"""
    if forced:
        monkeypatch.setenv("SF_AMD_PREC_GROUPS", "16")
        assert [pgrp_bytes(n, t, V) for t in (16, 8, 4, 2)] == [60816, 31888, 17424, 10192]
    else:
        assert default_trials(n, V) == 2 and pgrp_bytes(n, 2, V) == 14304
    p = _graph(n, n // 2, V, seed=9)
    assert 28 * n + 8 * (n // 2) + 24 == (9624 if forced else 13720)
    _window(oracle, p, dict(LDS, prec_static=1, prec_groups=T, prec_occ=False), capacity=capacity)


# ---- MODE 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,occ", [(2048, False), (2049, True)])
def test_mode2_replica_edge(oracle, R, occ):
    """30 x 20 shop (600 nodes: slim copy, no groups; slice 9,424 bytes = 16 per CU) under default settings: 2,048 replicas keep the
    two-workgroups-per-CU build, 2,049 take MODE 2 -- k_mixed_search_wave<2, false, int16_t, false, true, 2>."""
    from solverforge_amd import datasets

    p = datasets.make_precedence_shop(30, 20, seed=9)
    _window(oracle, p, dict(LDS, prec_static=2, prec_groups=0, prec_occ=occ), leaves=("list_change", "list_swap"), R=R, replicas=(0, 1, R // 2, R - 1))


def test_mode2_nine_leaf_policy_on_the_benchmarked_shop(oracle):
    """The benchmarked 50 x 20 shop under the nine-leaf policy with the slot's precedence hooks at 2,049 replicas: slice 16,080 bytes, ten per
    CU -- the PREC + RUIN MODE 2 instantiation k_mixed_search_wave<2, false, int16_t, true, true, 2>."""
    from solverforge_amd import datasets

    p = datasets.make_precedence_shop(50, 20, seed=1)
    R = 2049
    # (the oracle prices a candidate of this policy at 1,000 nodes in about 0.25 s: two steps of at most four accepted candidates per replica)
    _window(oracle, p, dict(LDS, prec_static=2, prec_groups=0, prec_occ=True, ruin_inst=True), leaves=NINE, policy=True, R=R, replicas=(0, 1, 1024, R - 1),
            steps=2, la=5, limit=4)


def test_mode2_three_level_model(oracle):
    """Three score levels (the L = 4 template) in MODE 2: 30 x 20 shop, 2,049 replicas."""
    from solverforge_amd import datasets

    p = datasets.make_precedence_shop(30, 20, seed=10)
    R = 2049
    _window(oracle, p, dict(LDS, prec_static=2, prec_groups=0, prec_occ=True, levels=4), leaves=("list_change", "list_swap"), R=R, replicas=(0, 1, 1000, R - 1),
            levels=3)


@pytest.mark.parametrize("n,occ", [(1217, True), (1218, False)])
def test_mode2_slice_edge(oracle, n, occ):
    """8 lists, two leaves: 1,217 nodes give a slice of 17,936 bytes (163,840 / 18,192 = 9 per CU: MODE 2), 1,218 nodes 17,952 (8: MODE 0)."""
    p = _graph(n, n // 2, 8, seed=11)
    R = 2049
    _window(oracle, p, dict(LDS, prec_static=2, prec_groups=0, prec_occ=occ), leaves=("list_change", "list_swap"), R=R, replicas=(0, 1, 1024, R - 1), steps=3)


# ---- one-byte values under PREC -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bendable,n_ops,n_machines,vb", [(False, 1024, 127, 1), (True, 1024, 127, 1), (True, 1023, 127, 2), (True, 1024, 128, 2)])
def test_one_byte_values_under_prec(oracle, bendable, n_ops, n_machines, vb):
    """The mixed job shop with the makespan objective: 1,024 scalar entities over 127 values run k_mixed_search_wave<L, *, int8_t, false, true, 0>,
    with the two-level score (hard / soft: the L = 2 template) and with the bendable three-level one (the L = 4 template); there 1,023
    entities or 128 values run the int16_t one.  Traced steps, then a fused window."""
    import solverforge_amd as sfa
    from solverforge_amd import datasets

    ids = np.arange(n_ops, dtype=np.int64)
    p = {"n_ops": n_ops, "n_machines": n_machines, "job": ids // 8, "step": ids % 8, "machine_idx": np.full(n_ops, -1, dtype=np.int64),
         "sequences": [[] for _ in range(n_machines)]}
    p = datasets.construct_jobshop(p, seed=3)
    p["durations"] = (datasets.stream(5, n_ops) % np.uint64(9)).astype(np.int64) + 1
    p["sequences"][2] = p["sequences"][2][::-1]
    d = sfa.build_jobshop(p, makespan=True, bendable=bendable)
    o = oracle.Model.jobshop(p["job"], p["machine_idx"], p["sequences"], bendable=bendable, durations=p["durations"])
    L = 3 if bendable else 2
    assert (d.calculate_score()[0] == o.score()[:L]).all()
    gs, gc = d.evaluate_each()
    os_, oc = o.evaluate_each()
    assert (gs == os_[:, :L]).all() and (gc == oc).all()
    o.configure(leaves=4 | 8 | 1 | 2, random_seed=2, la_size=5, limit=12)
    d.configure(sfa.SolverConfig(random_seed=2, late_acceptance_size=5, accepted_count_limit=12))
    d.phase_start()
    o.phase_start()
    # (128 lists: no grouped evaluator; 1,024 nodes without owners: the slim copy)
    want = dict(LDS, prec_static=2, prec_groups=0, prec_occ=False, value_bytes=vb, levels=4 if bendable else 2)
    for step in range(3):
        gm, gsc, gf, gap, gmv = d.solve_step_traced(cap=1 << 18)
        om, osc, of, oap, omv = o.step_traced()
        assert len(gm) == len(om), step
        assert (_t(gm) == _t(om)).all() and (gf == of).all() and (gsc == osc[:, :L]).all(), step
        assert gap == oap and (not gap or tuple(gmv) == tuple(omv)), step
    _placed(d, want)
    d.solve_steps(4)
    o.steps(4)
    _placed(d, want)
    assert d.working_lists(1, 0) == o.get_lists(1)
    assert (d.working_values(0, 0) == o.get_vars(0, 0)).all()
    assert (d.calculate_score()[0] == o.score()[:L]).all() and (d.best_scores()[0] == o.best_score()[:L]).all()
    assert (d.fresh_score()[0] == o.score()[:L]).all()
    gst, ost = d.stats(0), o.stats()
    for c in COUNTERS:
        assert gst[c] == ost[c], c
