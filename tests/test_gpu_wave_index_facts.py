"""GPU parity tests of the run-time unit compiled for the facts of the neighbour index, after tests/test_gpu_wave_spec.py: the same
fused solve of three launches under SF_AMD_WAVE_SPEC = 0 (the ahead-of-time kernel) and = 1 with SF_AMD_WAVE_SPEC_EXTRAS selecting each
candidate alone and all four together.  Every list, score, best snapshot, LateAcceptance slot and cursor and sf_stats word must be equal in
every replica, and replica 0 must equal the CPU oracle.

The matrices are built row by row so that every row of the index has the equal-distance groups a case names (the node itself first, then
the other nodes in a seeded order, distances = the group's number): groups across lanes 15 | 16 and 31 | 32, groups left open at entry 31
and at entry 63, widths 2, 3 and 5 in one row, widths 33 and 63, width 64 and an all-equal matrix (the facts must keep the serial top-k and
say so), no ties at all, rows shorter than a half.  Each case first checks, through sf_debug_nbr_facts and on the flags themselves, that the
index built the way k_nbr_presort builds it has that structure, and after every launch that the key names the facts and exactly the
candidates they allow."""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_wave_spec as ws

pytestmark = pytest.mark.gpu

X_DEFAULT, X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL, X_INDEX_ALL = 11, 32, 64, 128, 256, 480
END, SAME = 0xFFFF, 0x8000
KEY_WORDS = 22


def ones(n):
    return [1] * n


# name: (customers, vehicles, max_nearby, group widths of every row -- padded with single entries to the row's length)
CASES = {
    "across_lanes_15_16": (99, 5, 20, ones(14) + [4]),           # entries 14 .. 17
    "across_lanes_31_32_open_at_31": (80, 4, 32, ones(30) + [4]),  # entries 30 .. 33: open at the end of a half, closed by gen_rest
    "open_at_63": (129, 8, 32, ones(20) + [3] + ones(39) + [4]),   # entries 62 .. 65: open at the end of gen_rest's first chunk
    "widths_2_3_5": (70, 3, 20, [1, 2, 1, 3, 1, 5, 2, 2, 3]),
    "widths_2_3_5_k1": (70, 3, 1, [1, 2, 1, 3, 1, 5, 2, 2, 3]),
    "width_33": (90, 6, 32, [1, 33]),                              # wider than a half
    "width_63": (100, 7, 20, [1, 63, 2]),
    "width_64": (110, 5, 20, [1, 64]),                             # wide_ties: the serial top-k stays
    "all_equal": (75, 4, 20, [76]),
    "no_ties": (85, 5, 20, []),
    "no_ties_k32": (72, 3, 32, []),
    "rows_shorter_than_a_half": (19, 3, 20, [1, 2, 3]),            # 20 entries a row: every lane from 20 on is past its row
}


def _matrix(dim, widths, seed):
    widths = list(widths) + ones(dim - sum(widths))
    assert sum(widths) == dim and widths[0] >= 1
    dist = np.repeat(np.arange(len(widths), dtype=np.int64), widths)
    rng = np.random.default_rng(seed)
    mat = np.zeros((dim, dim), dtype=np.int64)
    for r in range(dim):
        others = rng.permutation(np.delete(np.arange(dim), r))
        mat[r, np.concatenate([[r], others])] = dist  # the node itself is entry 0
    return mat, widths


def _index(mat):
    """k_nbr_presort on the host: every row sorted by (distance, node), bit 15 = same distance as the entry before."""
    dim = mat.shape[0]
    keys = np.empty((dim, dim), dtype=np.uint16)
    for r in range(dim):
        order = np.lexsort((np.arange(dim), mat[r]))
        d = mat[r, order]
        keys[r] = order.astype(np.uint16) | np.where(np.concatenate([[False], d[1:] == d[:-1]]), SAME, 0).astype(np.uint16)
    return keys


def _facts(keys):
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_nbr_facts.restype = ctypes.c_int32
    out = (ctypes.c_int32 * 2)()
    assert L.sf_debug_nbr_facts(keys.ctypes.data_as(ctypes.c_void_p), keys.shape[0], keys.shape[1], out, 2) == 0
    return out[0], out[1]


def _key22(d):
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_wave_spec.restype = ctypes.c_int32
    out = (ctypes.c_int32 * (4 + KEY_WORDS))()
    assert L.sf_debug_wave_spec(d._h, out, len(out)) == 0
    return list(out)


def _allowed(V, dim, n_cap, tie_max, rows_full):
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_wave_spec_index_gate.restype = ctypes.c_int32
    return L.sf_debug_wave_spec_index_gate((ctypes.c_int32 * 5)(V, dim, n_cap, tie_max, rows_full), 5)


def _solve(spec, p, knob, extras):
    """The three launches under SF_AMD_WAVE_SPEC = knob and SF_AMD_WAVE_SPEC_EXTRAS = extras; the 22-word report after each; the state left behind."""
    d = ws._director(spec, p)
    said = []
    os.environ["SF_AMD_WAVE_SPEC"], os.environ["SF_AMD_WAVE_SPEC_EXTRAS"] = knob, str(extras)
    try:
        for n in ws.LAUNCHES:
            d.solve_steps(n)
            said.append(_key22(d))
    finally:
        del os.environ["SF_AMD_WAVE_SPEC"], os.environ["SF_AMD_WAVE_SPEC_EXTRAS"]
    mode = d.wave_layout()[0]
    reps = ws._snapshot(d, spec)
    d.close()
    return mode, said, reps


@pytest.mark.parametrize("name", list(CASES))
def test_index_structures(name, oracle):
    from solverforge_amd import datasets

    customers, vehicles, max_nearby, widths = CASES[name]
    dim = customers + 1
    spec = ws._spec(customers, vehicles, max_nearby=max_nearby)
    p = datasets.make_cvrp(customers, vehicles, spec["capacity"], seed=3)
    p["matrix"], widths = _matrix(dim, widths, seed=len(name))
    # the index really has the structure the case was built for
    keys = _index(p["matrix"])
    flags = np.repeat(False, dim)
    flags[np.setdiff1d(np.arange(dim), np.cumsum([0] + widths[:-1]))] = True
    assert ((keys & SAME != 0) == flags[None, :]).all() and (keys != END).all()
    tie_max, rows_full = _facts(keys)
    assert (tie_max, rows_full) == (min(max(widths), 64), 1)
    starts = np.cumsum([0] + widths[:-1])
    covers = lambda a, b: any(s <= a and s + w > b for s, w in zip(starts, widths))  # one group holds entries a and b
    want = {"across_lanes_15_16": covers(15, 16), "across_lanes_31_32_open_at_31": covers(31, 32), "open_at_63": covers(63, 64), "widths_2_3_5": {2, 3, 5} <= set(widths[:8]),
            "widths_2_3_5_k1": {2, 3, 5} <= set(widths[:8]), "width_33": 33 in widths, "width_63": tie_max == 63, "width_64": tie_max == 64 and max(widths) == 64,
            "all_equal": widths == [dim] and tie_max == 64, "no_ties": tie_max == 1, "no_ties_k32": tie_max == 1, "rows_shorter_than_a_half": dim < 32}
    assert want[name]
    allowed = _allowed(vehicles, dim, customers, tie_max, rows_full)
    assert bool(allowed & X_NO_WIDE) == (tie_max < 64) and bool(allowed & X_NO_TIES) == (tie_max < 2) and bool(allowed & X_ROWS_FULL) == (dim >= 32) and allowed & X_TIE_KEY

    mode, said, ref = _solve(spec, p, "0", X_DEFAULT)
    assert mode == 5 and all((s[0], s[1]) == (ws.AOT, ws.R_KNOB) for s in said)
    seen = set()
    for bits in (X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL, X_INDEX_ALL):
        mode, said, got = _solve(spec, p, "1", X_DEFAULT | bits)
        for s in said:
            # the specialised kernel ran, its key names the facts and the candidates the facts allow -- never one they do not
            assert mode == 5 and (s[0], s[1]) == (ws.SPECIALISED, 0), (bits, s)
            assert s[4 + 7] == X_DEFAULT and s[4 + 18:] == [int(tie_max >= 64), int(tie_max >= 2), 1, bits & allowed], (bits, s)
        seen.add(bits & allowed)
        for r, (a, b) in enumerate(zip(ref, got)):
            for word in a:
                assert a[word] == b[word], (bits, r, word)  # lists, scores, best snapshot, every history slot and its cursor, every sf_stats word
    assert seen >= {allowed & b for b in (X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL)}

    o = oracle.Model.cvrp(p["capacity"], p["depot"], p["demands"], p["matrix"], p["customers"], p["routes"])
    o.configure(la_size=spec["la"], limit=256, leaves=oracle.LEAF_NEARBY_LIST_CHANGE | oracle.LEAF_NEARBY_LIST_SWAP, max_nearby=max_nearby, random_seed=spec["seed"])
    o.phase_start()
    o.steps(sum(ws.LAUNCHES))
    g = ref[0]
    assert g["score"] == [int(x) for x in o.score()[:2]] and g["fresh"] == g["score"] and g["best"] == [int(x) for x in o.best_score()[:2]] and g["lists"] == o.get_lists(0)
    for k in ws.ORACLE_WORDS:
        assert g["stats"][k] == o.stats()[k], k
