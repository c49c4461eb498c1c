"""GPU: the GreatDeluge and StepCountingHillClimbing code of the search engines (csrc/sf_step.h: acceptor_phase_started, step_begin,
acceptor_accepts, acceptor_step_ended) alone, through sf_debug_acceptor_script, against tests/acceptor_mirror.py: every golden sequence
of the reference's unit tests and every hand-written edge script (tests/test_acceptor_mirror.py pins both on the CPU), 64 candidates per
decide record that straddle the threshold.  Every accept ballot and every state word after every record must be the mirror's."""
import numpy as np
import pytest

import acceptor_mirror as am

pytestmark = pytest.mark.gpu

_ctx = {}


def _director():
    """Device and stream only: the entry point needs no model."""
    if "d" not in _ctx:
        import solverforge_amd as sfa

        _ctx["d"] = sfa.GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=1)
    return _ctx["d"]


def _records(plan):
    from solverforge_amd._lib import ACCEPTOR_RECORD_DTYPE

    rec = np.zeros(len(plan), dtype=ACCEPTOR_RECORD_DTYPE)
    for i, p in enumerate(plan):
        rec[i]["op"] = p["op"]
        rec[i]["cur"] = p["cur"]
        rec[i]["doable"] = p["doable"]
        if p["sc"] is not None:
            rec[i]["sc"] = p["sc"]
    return rec


@pytest.mark.parametrize("script", am.all_scripts(), ids=lambda s: s["name"])
def test_script_matches_the_mirror(script):
    import solverforge_amd as sfa

    plan = am.device_plan(script)
    gd = script["acceptor"] == "great_deluge"
    kind = sfa.Acceptor.GREAT_DELUGE if gd else sfa.Acceptor.STEP_COUNTING_HILL_CLIMBING
    accept, state = _director().debug_acceptor_script(kind, _records(plan), levels=script["levels"], rain_speed=script["param"] if gd else 0.0,
                                                      step_count_limit=0 if gd else script["param"])
    assert len(accept) == len(plan) and state.shape == (len(plan), 9)
    for i, p in enumerate(plan):
        assert int(accept[i]) == p["accept"], (i, p["op"], hex(int(accept[i])), hex(p["accept"]))
        level, incr, since = p["state"]
        got = state[i].view(np.int64)
        assert tuple(int(x) for x in got[0:4]) == level, (i, p["op"])
        assert tuple(int(x) for x in got[4:8]) == incr, (i, p["op"])
        assert int(state[i][8]) == since, (i, p["op"])


def test_validation():
    import solverforge_amd as sfa

    d = _director()
    rec = _records(am.device_plan(am.goldens()[0]))
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_acceptor_script(sfa.Acceptor.LATE_ACCEPTANCE, rec, levels=1)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_acceptor_script(sfa.Acceptor.GREAT_DELUGE, rec, levels=1, rain_speed=float("inf"))
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_acceptor_script(sfa.Acceptor.GREAT_DELUGE, rec, levels=5)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_acceptor_script(sfa.Acceptor.GREAT_DELUGE, rec[1:], levels=1)  # the first record must start the phase
