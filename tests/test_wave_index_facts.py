"""CPU tests of the facts of the neighbour index the wave engine's run-time unit may be compiled for: the host reduction
(csrc/sf_nbr_facts.h through sf_debug_nbr_facts) against a numpy reduction on hand-built indexes, the candidates' gate
(wave_spec_index_allowed through sf_debug_wave_spec_index_gate) on both sides of every fact and of the packed word's width, the option list of
each new bit, and the unit compiled for gfx950 through hiprtc without a device for the benchmark's key with each candidate alone and with all
of them: one kernel, no scratch, at most 80 vector registers."""
import ctypes

import numpy as np
import pytest

from test_wave_spec import BENCH_KEY, KEY, R_NONE, SF_ERR_INVALID, kernel_notes

KEY22 = KEY + ["wide_ties", "ties", "rows_full", "index_x"]  # WaveSpecKey, declaration order
X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL = 32, 64, 128, 256
END, SAME = 0xFFFF, 0x8000
# the benchmark's model words (the default candidates of DESIGN 22) and its index's facts: ties everywhere, none wider than 11, no short row
BENCH_DEFAULT = dict(BENCH_KEY, extras=11, capacity=55, cap_weight=1, dist_weight=1, depot=0, cap_level=0, dist_level=1, la_size=400, has_perm=1)
BENCH_FACTS = dict(wide_ties=0, ties=1, rows_full=1)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    for f in ("sf_debug_nbr_facts", "sf_debug_wave_spec_index_gate", "sf_debug_wave_spec_compile"):
        getattr(L, f).restype = ctypes.c_int32
    return L


# ---- the reduction ------------------------------------------------------------------------------------------------------------------------------
def row_of(widths, dim, first_node=0):
    """One index row: groups of the given widths, then end marks up to `dim`."""
    out, node = [], first_node
    for w in widths:
        for i in range(w):
            out.append(node | (SAME if i else 0))
            node += 1
    assert len(out) <= dim
    return out + [END] * (dim - len(out))


def np_facts(keys):
    keys = np.asarray(keys, dtype=np.uint16)
    finite = keys != END
    cont = finite & ((keys & SAME) != 0)
    cont[:, 0] = False
    run = np.zeros(keys.shape[0], dtype=np.int64)
    widest = 0
    for t in range(keys.shape[1]):
        run = np.where(cont[:, t], run + 1, finite[:, t].astype(np.int64))
        widest = max(widest, int(run.max()))
    return min(widest, 64), int((finite.sum(axis=1) >= min(keys.shape[1], 64)).all())


def facts(lib, keys):
    a = np.ascontiguousarray(np.asarray(keys, dtype=np.uint16))
    out = (ctypes.c_int32 * 2)()
    assert lib.sf_debug_nbr_facts(a.ctypes.data_as(ctypes.c_void_p), a.shape[0], a.shape[1], out, 2) == 0
    return out[0], out[1]


INDEXES = {
    "no_ties": ([row_of([1] * 100, 100), row_of([1] * 100, 100)], (1, 1)),
    "width_2": ([row_of([1] * 98, 100), row_of([1] * 40 + [2] + [1] * 58, 100)], (2, 1)),
    "width_63": ([row_of([1, 63] + [1] * 36, 100), row_of([1] * 100, 100)], (63, 1)),
    "width_64": ([row_of([1] * 100, 100), row_of([3, 64] + [1] * 33, 100)], (64, 1)),
    "width_65": ([row_of([65] + [1] * 35, 100)], (64, 1)),
    "width_100_all_equal": ([row_of([100], 100)] * 3, (64, 1)),
    "a_row_of_31": ([row_of([1] * 100, 100), row_of([1] * 31, 100)], (1, 0)),
    "a_row_of_32": ([row_of([1] * 32, 100), row_of([1] * 100, 100)], (1, 0)),
    "a_row_of_63": ([row_of([1] * 100, 100), row_of([2] + [1] * 61, 100)], (2, 0)),
    "a_row_of_64_of_100": ([row_of([1] * 64, 100)], (1, 1)),
    "dim_below_32_full": ([row_of([1] * 20, 20), row_of([5] + [1] * 15, 20)], (5, 1)),
    "dim_below_32_short": ([row_of([1] * 20, 20), row_of([1] * 19, 20)], (1, 0)),
    "flag_on_an_end_mark_is_no_tie": ([row_of([1, 1], 5)], (1, 0)),  # 0xFFFF carries bit 15: an end mark continues nothing
    "no_finite_entry": ([[END] * 8], (0, 0)),
}


@pytest.mark.parametrize("name", list(INDEXES))
def test_facts_against_numpy(lib, name):
    keys, want = INDEXES[name]
    assert np_facts(keys) == want  # the hand-built index has the structure it was built for
    assert facts(lib, keys) == want


def test_facts_of_a_sorted_random_matrix(lib):
    """An index built the way k_nbr_presort builds it, from a matrix with few distinct distances and some unreachable legs."""
    rng = np.random.default_rng(11)
    dim = 90
    mat = rng.integers(0, 12, size=(dim, dim))
    mat[rng.random((dim, dim)) < 0.3] = -1
    keys = np.full((dim, dim), END, dtype=np.uint16)
    for r in range(dim):
        order = sorted((int(v), t) for t, v in enumerate(mat[r]) if v >= 0)
        for i, (v, t) in enumerate(order):
            keys[r, i] = t | (SAME if i and order[i - 1][0] == v else 0)
    assert facts(lib, keys) == np_facts(keys)
    assert np_facts(keys)[0] >= 2 and np_facts(keys)[1] == 0


def test_facts_refuse_bad_arguments(lib):
    a = np.zeros((2, 2), dtype=np.uint16)
    out = (ctypes.c_int32 * 2)()
    p = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.sf_debug_nbr_facts(None, 2, 2, out, 2) == SF_ERR_INVALID
    assert lib.sf_debug_nbr_facts(p, 0, 2, out, 2) == SF_ERR_INVALID and lib.sf_debug_nbr_facts(p, 2, 0, out, 2) == SF_ERR_INVALID
    assert lib.sf_debug_nbr_facts(p, 2, 2, out, 3) == SF_ERR_INVALID


# ---- the gate -----------------------------------------------------------------------------------------------------------------------------------
def allowed(lib, V=100, dim=1001, n_cap=1000, tie_max=11, rows_full=1):
    return lib.sf_debug_wave_spec_index_gate((ctypes.c_int32 * 5)(V, dim, n_cap, tie_max, rows_full), 5)


def test_gate_of_the_benchmark(lib):
    assert allowed(lib) == X_NO_WIDE | X_TIE_KEY | X_ROWS_FULL


def test_gate_wide_ties(lib):
    assert allowed(lib, tie_max=63) & X_NO_WIDE and not allowed(lib, tie_max=64) & X_NO_WIDE


def test_gate_ties(lib):
    assert allowed(lib, tie_max=1) & X_NO_TIES and allowed(lib, tie_max=0) & X_NO_TIES and not allowed(lib, tie_max=2) & X_NO_TIES


def test_gate_rows_full(lib):
    assert allowed(lib, rows_full=1) & X_ROWS_FULL and not allowed(lib, rows_full=0) & X_ROWS_FULL
    assert allowed(lib, dim=32) & X_ROWS_FULL and not allowed(lib, dim=31) & X_ROWS_FULL  # the paired pass reads 32 entries of a row


@pytest.mark.parametrize("V,n_cap,fits", [(100, 1000, True), (1022, 4095, True), (1022, 4096, False), (512, 8191, True), (513, 8191, False), (512, 8192, False), (1, 1, True)])
def test_gate_packed_word(lib, V, n_cap, fits):
    """RB + PB <= 22: RB = the bits that hold V - 1, PB = the bits that hold n_cap.  1021 -> 10, 4095 -> 12 / 4096 -> 13; 511 -> 9 / 512 -> 10, 8191 -> 13."""
    rb, pb = max(1, int(V - 1).bit_length()), max(1, int(n_cap).bit_length())
    assert (rb + pb <= 22) == fits
    assert bool(allowed(lib, V=V, n_cap=n_cap) & X_TIE_KEY) == fits


def test_gate_refuses_other_sizes(lib):
    assert lib.sf_debug_wave_spec_index_gate((ctypes.c_int32 * 4)(), 4) == SF_ERR_INVALID


# ---- the option list and the unit ---------------------------------------------------------------------------------------------------------------
def compile_key(lib, key, out_path=None):
    k = (ctypes.c_int32 * len(KEY22))(*[key.get(n, 0) for n in KEY22])
    opts, log, ms = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(1 << 16), ctypes.c_double(0)
    rc = lib.sf_debug_wave_spec_compile(k, len(KEY22), b"gfx950", None if out_path is None else str(out_path).encode(), opts, len(opts), log, len(log), ctypes.byref(ms))
    return rc, opts.value.decode().split("\n")[:-1], log.value.decode(errors="replace"), ms.value


WANT = {X_NO_WIDE: ["-DSF_SPEC_NO_WIDE=(1)"], X_TIE_KEY: ["-DSF_SPEC_TIE_KEY=(1)", "-DSF_SPEC_RB=(7)", "-DSF_SPEC_PB=(10)"], X_NO_TIES: ["-DSF_SPEC_NO_TIES=(1)"],
        X_ROWS_FULL: ["-DSF_SPEC_ROWS_FULL=(1)"]}
NO_TIE_FACTS = dict(wide_ties=0, ties=0, rows_full=1)  # the benchmark's constants over an index without ties: every candidate is allowed


def test_options_of_the_candidates(lib):
    """Each candidate behind its own bit: nothing of one that is off reaches the compiler, and the facts alone add nothing."""
    for mask in (0, X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL, 480):
        rc, opts, _, _ = compile_key(lib, dict(BENCH_KEY, **NO_TIE_FACTS, index_x=mask))
        assert rc == R_NONE
        assert [o for o in opts if o.startswith("-D")][7:] == [o for bit in (X_NO_WIDE, X_TIE_KEY, X_NO_TIES, X_ROWS_FULL) if mask & bit for o in WANT[bit]], mask
    rc, opts, _, _ = compile_key(lib, dict(BENCH_DEFAULT, **BENCH_FACTS, index_x=X_TIE_KEY))
    assert rc == R_NONE and opts[-3:] == WANT[X_TIE_KEY]  # after the candidates of the model's constants


def test_a_candidate_its_facts_do_not_allow_is_refused(lib):
    for bad in (dict(wide_ties=1, ties=1, index_x=X_NO_WIDE), dict(ties=1, index_x=X_NO_TIES), dict(rows_full=0, index_x=X_ROWS_FULL), dict(rows_full=1, dim=31, index_x=X_ROWS_FULL),
                dict(V=1022, n_cap=4096, index_x=X_TIE_KEY), dict(index_x=512), dict(index_x=1), dict(wide_ties=1, ties=0), dict(ties=2)):
        assert compile_key(lib, dict(BENCH_KEY, **dict(NO_TIE_FACTS, **bad)))[0] == SF_ERR_INVALID, bad


UNITS = {
    "no_wide": dict(BENCH_DEFAULT, **BENCH_FACTS, index_x=X_NO_WIDE),
    "tie_key": dict(BENCH_DEFAULT, **BENCH_FACTS, index_x=X_TIE_KEY),
    "rows_full": dict(BENCH_DEFAULT, **BENCH_FACTS, index_x=X_ROWS_FULL),
    "no_ties": dict(BENCH_DEFAULT, **NO_TIE_FACTS, index_x=X_NO_TIES),  # (the benchmark's own index has ties: its constants over one that has none)
    "all_the_benchmark_allows": dict(BENCH_DEFAULT, **BENCH_FACTS, index_x=X_NO_WIDE | X_TIE_KEY | X_ROWS_FULL),
    "all_four": dict(BENCH_DEFAULT, **NO_TIE_FACTS, index_x=480),
    "all_four_on_the_floor": dict(BENCH_KEY, **NO_TIE_FACTS, index_x=480),
}


@pytest.mark.parametrize("name", list(UNITS))
def test_unit_compiles_without_a_device(lib, tmp_path, name):
    co = tmp_path / "spec.co"
    rc, _, log, ms = compile_key(lib, UNITS[name], co)
    assert rc == R_NONE, log[-4000:]
    ks = kernel_notes(co)
    assert len(ks) == 1 and "k_list_search_wave" in ks[0][".name"], [k[".name"] for k in ks]
    k = ks[0]
    print("compile ms", round(ms), {f: k[f] for f in (".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size")})
    assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".vgpr_spill_count"]) == 0  # no scratch
    assert int(k[".vgpr_count"]) <= 80
