"""GPU test (through the C ABI): the SimulatedAnnealing acceptor of the search engines alone, chunk by chunk, against the oracle's
acceptor.  sf_debug_anneal_chunks runs sa_decide / sa_commit / sa_step_ended of csrc/sf_anneal.h -- the code all four engines
inline -- on the scripted sequences of tests/anneal_chunk_cases.py, one launch of one wave per sequence; every consumed
candidate's accept flag, the rng words, the calibrating flag, the temperatures as bit patterns, samples_seen and the per-level
sample count and 128-bit total are compared after every chunk and after every step end.

tests/test_anneal_chunk_cases.py proves on the oracle alone which edges the sequences reach and that none of them contains a draw
within 4 spacings of its probability (the tie rule), so nothing here is compared with a tolerance.  Not reached by any test: the
sh == 64 arm of sa_u128_to_f64 (a total of 2^127 or more; an int32 sample count keeps totals below 2^94)."""
import numpy as np
import pytest

import anneal_chunk_cases as cases

pytestmark = pytest.mark.gpu

GROUPS = ("calib-", "cut-", "total-", "delta-", "temp-", "levels-", "long-mixed-L2", "long-mixed-L4")


@pytest.fixture(scope="module")
def device():
    from solverforge_amd.director import GpuScoreDirector

    return GpuScoreDirector()  # a context without a model: the harness takes its device and stream only


def test_groups_cover_every_sequence():
    for s in cases.sequences():
        assert sum(s.name.startswith(g) for g in GROUPS) == 1, s.name


@pytest.mark.parametrize("group", GROUPS)
def test_acceptor_chunks_match_oracle(oracle, device, group):
    seqs = [s for s in cases.sequences() if s.name.startswith(group)]
    assert seqs
    for seq in seqs:
        rep = cases.replay_oracle(oracle, seq)
        accept, state = device.debug_anneal_chunks(seq.chunks, **seq.device_kwargs())
        cases.compare_device(seq, rep, accept, state)


def test_harness_validates_its_arguments(device):
    import solverforge_amd as sfa

    one = np.zeros(1, dtype=cases.ANNEAL_CHUNK_DTYPE)
    one["nconsumed"] = 64
    device.debug_anneal_chunks(one)
    bad_chunk = one.copy()
    bad_chunk["nconsumed"] = 65
    neg_chunk = one.copy()
    neg_chunk["nconsumed"] = -1
    for chunks, kw in [(one, dict(levels=0)), (one, dict(levels=5)), (one, dict(levels=2, hard_levels=3)), (one, dict(hard_levels=-1)),
                       (one[:0], {}), (bad_chunk, {}), (neg_chunk, {}), (one, dict(decay_rate=0.0)), (one, dict(mode=3)),
                       (one, dict(calibration_sample_size=0)), (one, dict(mode=1, levels=3, hard_levels=1, temperatures=(1.0, 1.0, -1.0))),
                       (np.zeros(65537, dtype=cases.ANNEAL_CHUNK_DTYPE), {})]:
        with pytest.raises(sfa.SolverForgeError, match="SF_ERR_INVALID"):
            device.debug_anneal_chunks(chunks, **kw)
    device.debug_anneal_chunks(one, mode=1, levels=2, temperatures=(1.0, 1.0, -1.0))  # a temperature past the score's levels is not read
