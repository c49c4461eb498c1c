"""GPU: the TabuSearch code of the search engines (csrc/sf_tabu.h: tabu_phase_started, tabu_step_begin, tabu_accepts, tabu_step_ended)
alone, through sf_debug_tabu_script, against tests/tabu_mirror.py: every golden sequence of the reference's unit tests and every
hand-written edge script (tests/test_tabu_mirror.py pins both on the CPU).  Every decide record carries 64 candidates that straddle the
rule -- tabu by each memory alone, by several, by none, scores on both sides of the acceptor's best, lanes masked off.  Every ballot and
every state word after every record must be the mirror's."""
import numpy as np
import pytest

import tabu_mirror as tm

pytestmark = pytest.mark.gpu

_ctx = {}


def _director():
    """Device and stream only: the entry point needs no model."""
    if "d" not in _ctx:
        import solverforge_amd as sfa

        _ctx["d"] = sfa.GpuScoreDirector(score_levels=2, hard_levels=1, n_replicas=1)
    return _ctx["d"]


def _records(plan):
    from solverforge_amd._lib import TABU_RECORD_DTYPE

    rec = np.zeros(len(plan), dtype=TABU_RECORD_DTYPE)
    rec["sig"]["entity"] = tm.NO_TOKEN
    rec["sig"]["value"] = tm.NO_TOKEN
    for i, p in enumerate(plan):
        rec[i]["op"] = p["op"]
        rec[i]["score"] = p["score"]
        rec[i]["reach"] = p["reach"]
        sigs = [s for s, _ in p["cands"]] if p["cands"] is not None else ([p["sig"]] if p["sig"] is not None else [])
        rec[i]["has_sig"] = 1 if p["sig"] is not None else 0
        for lane, s in enumerate(sigs):
            for k in ("entity", "value", "move_id", "undo_move_id"):
                rec[i]["sig"][lane][k] = s[k]
        if p["cands"] is not None:
            rec[i]["sc"] = [c for _, c in p["cands"]]
    return rec


def _policy_kwargs(script):
    e, v, m, u, asp = tm.normalize_policy(script["policy"])
    return dict(entity_tabu_size=e, value_tabu_size=v, move_tabu_size=m, undo_move_tabu_size=u, aspiration_enabled=asp)


def decode_state(row, n_ent, n_val):
    """A state row of sf_debug_tabu_script in the mirror's terms: (best[4], pushes[4], tabu entity tokens, tabu value tokens, move ids
    oldest first, undo ids oldest first)."""
    row = [int(x) for x in row]
    best = tuple(x - (1 << 64) if x >= 1 << 63 else x for x in row[0:4])
    pushes, tenure = tuple(row[4:8]), row[8:12]
    sets = []
    for q, (base, n) in enumerate(((16, n_ent), (16 + n_ent, n_val))):
        stamps = row[base:base + n]
        sets.append([t for t, st in enumerate(stamps) if tenure[q] and st != 0 and pushes[q] - st < tenure[q]])
    rings = []
    for q in (2, 3):
        base = 16 + n_ent + n_val + (q - 2) * 128
        live = min(pushes[q], tenure[q])
        slots = range(live) if pushes[q] <= tenure[q] else [(pushes[q] + k) % tenure[q] for k in range(live)]
        rings.append([(row[base + 2 * s], row[base + 2 * s + 1]) for s in slots])
    return best, pushes, sets[0], sets[1], rings[0], rings[1]


@pytest.mark.parametrize("script", tm.all_scripts(), ids=lambda s: s["name"])
def test_script_matches_the_mirror(script):
    plan, packer = tm.device_plan(script)
    n_ent, n_val = max(1, len(packer.ent)), max(1, len(packer.val))
    accept, state = _director().debug_tabu_script(_records(plan), n_ent, n_val, levels=script["levels"], **_policy_kwargs(script))
    assert len(accept) == len(plan) and state.shape == (len(plan), 16 + n_ent + n_val + 256)
    want_tenures = [t or 0 for t in tm.normalize_policy(script["policy"])[:4]]
    for i, p in enumerate(plan):
        assert int(accept[i]) == p["accept"], (i, p["op"], hex(int(accept[i])), hex(p["accept"]))
        assert decode_state(state[i], n_ent, n_val) == p["state"], (i, p["op"])
        assert [int(x) for x in state[i][8:16]] == want_tenures + [1 if tm.normalize_policy(script["policy"])[4] else 0, 0, 0, 0], i


def test_zero_tenures_and_validation():
    import solverforge_amd as sfa

    d = _director()
    script = tm.goldens()[0]
    plan, packer = tm.device_plan(script)
    rec = _records(plan)
    for case in tm.policy_error_golden()["policy_errors"]:
        e, v, m, u, asp = case["policy"]
        with pytest.raises(sfa.SolverForgeError, match="INVALID") as err:
            d.debug_tabu_script(rec, 16, 16, levels=1, entity_tabu_size=e, value_tabu_size=v, move_tabu_size=m, undo_move_tabu_size=u, aspiration_enabled=asp)
        assert case["message"] in str(err.value)
        with pytest.raises(sfa.SolverForgeError, match="INVALID") as err:
            d.configure_tabu(e, v, m, u, asp)
        assert case["message"] in str(err.value)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
        d.debug_tabu_script(rec, 16, 16, levels=1, move_tabu_size=65)
    with pytest.raises(sfa.SolverForgeError, match="UNSUPPORTED"):
        d.configure_tabu(undo_move_tabu_size=65)
    d.configure_tabu(move_tabu_size=64, undo_move_tabu_size=64)
    d.configure_tabu()
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_tabu_script(rec, 16, 16, levels=5, entity_tabu_size=1)
    with pytest.raises(sfa.SolverForgeError, match="INVALID"):
        d.debug_tabu_script(rec[1:], 16, 16, levels=1, entity_tabu_size=1)  # the first record must start the phase
    with pytest.raises(sfa.SolverForgeError, match="INVALID.*token outside"):
        d.debug_tabu_script(rec, 1, 1, levels=1, entity_tabu_size=1)  # the records name more than one entity token
