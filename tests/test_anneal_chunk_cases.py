"""CPU test of the scripted acceptor sequences (tests/anneal_chunk_cases.py), on the oracle alone: no sequence contains an
undecidable draw (the tie rule), and every sequence reaches the edge it is named for -- so what tests/test_gpu_anneal_chunks.py
covers on the device can be checked without one."""
import numpy as np
import pytest

import anneal_chunk_cases as cases


@pytest.fixture(scope="module")
def replays(oracle):
    return {s.name: (s, cases.replay_oracle(oracle, s)) for s in cases.sequences()}


def test_no_sequence_contains_an_undecidable_draw(replays):
    """|u - probability| <= 4 spacings of the probability nowhere: the share of draws a device test may leave out is zero."""
    for name, (seq, rep) in replays.items():
        assert cases.undecidable_draws(rep) == [], name


def test_every_sequence_reaches_its_edge(replays):
    for seq, rep in replays.values():
        cases.check_expectations(seq, rep)


def test_the_set_covers_the_named_edges(replays):
    """Across the whole set: completion at lanes 0, 31, 32, 63 for every sample size at two and four levels, a non-zero high half
    of the total, a saturated sample, draws at every level index of the four-level runs, probabilities of exactly 0 and in the
    denormal range, and 10,000 draws in each long run."""
    done = {(s.params["sample_size"], s.levels, r.completes[1]) for s, r in replays.values() if s.name.startswith("calib-")}
    for S in cases.CALIB_SIZES:
        for L in (2, 4):
            for f in cases.CALIB_LANES:
                assert (S, L, f) in done, (S, L, f)
    assert any(int(st["total_hi"].max()) > 0 for s, r in replays.values() for st in r.after_commit)
    assert any(v == cases.INT64_MAX for s, r in replays.values() for _, v in r.samples)
    for name in ("long-mixed-L2", "long-mixed-L4"):
        seq, rep = replays[name]
        assert sum(int(d.sum()) for d in rep.drew) >= 10000
        assert sorted(set(rep.draw_levels)) == list(range(seq.levels))
        assert len(seq.chunks) >= 2000 and rep.completes is not None
    hard_draws = [r for s, r in replays.values() if s.levels == 4 and s.hard_levels >= 2 and {0, 1} <= set(r.draw_levels)]
    assert hard_draws  # hard-level draws of the four-level build
    probs = np.concatenate([p[d] for s, r in replays.values() for p, d in zip(r.prob, r.drew)])
    assert (probs == 0.0).any() and ((probs > 0.0) & (probs < np.finfo(np.float64).tiny)).any()


def test_oracle_acceptor_without_a_model_matches_the_model_bound_one(oracle):
    """The stand-alone handle is the acceptor a Model installs: same rng seeding, same reported state."""
    a = oracle.Annealer(mode=1, temperatures=(2.0, 30.0), seed=5)
    a.phase_started()
    st = a.state()
    want = np.zeros(4, dtype=np.uint64)
    oracle.lib().sfo_small_rng_seed(5, want.ctypes.data)
    assert (st["rng"] == want).all() and not st["calibrating"] and list(st["temperatures"]) == [2.0, 30.0, 0.0, 0.0]
    acc, drew, u, p = a.is_accepted([0, 0, 0, 0], [0, -30, 0, 0])
    assert drew and p == np.exp(-1.0) and acc == (u < p) and 0.0 <= u < 1.0
    assert a.is_accepted([0, 0, 0, 0], [0, 5, 0, 0]) == (True, False, 0.0, 0.0)
    assert (a.state()["rng"] != want).any()
