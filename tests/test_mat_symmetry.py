"""CPU tests of the fact of the compact distance matrix the wave engine's run-time unit may be compiled for: the host reduction
(csrc/sf_mat_facts.h through sf_debug_mat_sym) on hand-built matrices -- judged on the u16 words the kernel reads, not on the 64-bit entries --
the leg candidates' gate (wave_spec_leg_allowed through sf_debug_wave_spec_leg_gate), the key's validity rule for the new word and bits, the
option list of each bit, and the unit compiled for gfx950 through hiprtc without a device for the benchmark's key with each candidate alone
and with both: one kernel, no scratch, at most 80 vector registers."""
import ctypes

import numpy as np
import pytest

from test_wave_index_facts import BENCH_DEFAULT, BENCH_FACTS, KEY22, X_NO_WIDE, X_ROWS_FULL, X_TIE_KEY
from test_wave_spec import BENCH_KEY, R_NONE, SF_ERR_INVALID, kernel_notes

KEY23 = KEY22 + ["mat_sym"]  # WaveSpecKey, declaration order
X_SYM_ROWS, X_LEG_REAIM = 512, 1024
UNREACHABLE = np.iinfo(np.int64).max
BENCH_INDEX = X_NO_WIDE | X_TIE_KEY | X_ROWS_FULL  # the index candidates the benchmark's launch compiles in


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    for f in ("sf_debug_mat_sym", "sf_debug_wave_spec_leg_gate", "sf_debug_wave_spec_compile", "sf_debug_wave_spec_legs"):
        getattr(L, f).restype = ctypes.c_int32
    return L


# ---- the reduction ------------------------------------------------------------------------------------------------------------------------------
def sym(lib, mat):
    a = np.ascontiguousarray(np.asarray(mat, dtype=np.int64))
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    out = (ctypes.c_int32 * 1)(-1)
    assert lib.sf_debug_mat_sym(a.ctypes.data_as(ctypes.c_void_p), a.shape[0], out, 1) == 0
    return out[0]


def words(mat):
    """k_mat_compress16's rule in numpy: what the kernel reads."""
    m = np.asarray(mat, dtype=np.int64)
    return np.where((m >= 0) & (m < 0xFFFF), m, 0xFFFF).astype(np.uint16)


def symmetric_matrix(dim, seed=1):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 5000, size=(dim, dim), dtype=np.int64)
    m = np.triu(m, 1)
    return m + m.T


def with_entries(m, *entries):
    m = m.copy()
    for a, b, v in entries:
        m[a, b] = v
    return m


S = symmetric_matrix(70)  # (more than one 64 x 64 tile of the reduction)
MATRICES = {
    "symmetric": (S, 1),
    "symmetric_with_a_diagonal": (with_entries(S, (3, 3, 17), (69, 69, 4)), 1),  # (a node's leg to itself has no pair)
    "one_finite_pair_off_by_one": (with_entries(S, (40, 12, int(S[12, 40]) + 1)), 0),
    "off_by_one_across_tiles": (with_entries(S, (69, 1, int(S[1, 69]) + 1)), 0),
    "off_by_one_in_the_last_tile": (with_entries(S, (69, 68, int(S[68, 69]) + 1)), 0),
    "one_direction_not_finite": (with_entries(S, (5, 9, UNREACHABLE)), 0),
    "one_direction_negative": (with_entries(S, (9, 5, -1)), 0),
    "both_directions_not_finite": (with_entries(S, (5, 9, UNREACHABLE), (9, 5, UNREACHABLE)), 1),
    "asymmetric_pair_on_the_depot_row": (with_entries(S, (0, 33, int(S[33, 0]) + 7)), 0),
    "asymmetric_pair_on_the_depot_column": (with_entries(S, (33, 0, int(S[0, 33]) + 7)), 0),
    "dim_1": (np.array([[5]]), 1),
    "dim_2_symmetric": (np.array([[0, 9], [9, 0]]), 1),
    "dim_2_asymmetric": (np.array([[0, 9], [8, 0]]), 0),
    # symmetric only on the words: the two directions differ as 64-bit entries and compress to the same not-finite word
    "clamped_large_pair": (with_entries(S, (7, 50, 70_000), (50, 7, 80_000)), 1),
    "clamped_at_the_edge": (with_entries(S, (7, 50, 0xFFFF), (50, 7, UNREACHABLE)), 1),
    "clamped_negative_and_unreachable": (with_entries(S, (7, 50, -4), (50, 7, UNREACHABLE)), 1),
    "last_finite_word_against_the_first_clamped": (with_entries(S, (7, 50, 0xFFFE), (50, 7, 0xFFFF)), 0),
}


@pytest.mark.parametrize("name", list(MATRICES))
def test_fact_on_the_words_the_kernel_reads(lib, name):
    mat, want = MATRICES[name]
    w = words(mat)
    assert int((w == w.T).all()) == want  # the hand-built matrix has the structure it was built for
    assert sym(lib, mat) == want


def test_the_clamped_cases_differ_as_entries():
    for name in ("clamped_large_pair", "clamped_at_the_edge", "clamped_negative_and_unreachable"):
        m = MATRICES[name][0]
        assert not (m == m.T).all(), name


def test_fact_of_random_matrices(lib):
    rng = np.random.default_rng(4)
    for dim in (3, 64, 65, 129):
        m = symmetric_matrix(dim, seed=dim)
        assert sym(lib, m) == 1
        a, b = (int(x) for x in rng.choice(dim, 2, replace=False))
        assert sym(lib, with_entries(m, (a, b, int(m[b, a]) + 1))) == 0, (dim, a, b)


def test_fact_refuses_bad_arguments(lib):
    a = np.zeros((2, 2), dtype=np.int64)
    out = (ctypes.c_int32 * 1)()
    p = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.sf_debug_mat_sym(None, 2, out, 1) == SF_ERR_INVALID and lib.sf_debug_mat_sym(p, 0, out, 1) == SF_ERR_INVALID
    assert lib.sf_debug_mat_sym(p, 2, out, 2) == SF_ERR_INVALID and lib.sf_debug_mat_sym(p, 2, None, 1) == SF_ERR_INVALID
    assert lib.sf_debug_wave_spec_legs(None, (ctypes.c_int32 * 2)(), 2) == SF_ERR_INVALID


# ---- the gate and the key -----------------------------------------------------------------------------------------------------------------------
def test_gate(lib):
    """The re-aimed gathers rest on nothing; the source-side rows are never offered while the fact is false."""
    assert lib.sf_debug_wave_spec_leg_gate(0) == X_LEG_REAIM
    assert lib.sf_debug_wave_spec_leg_gate(1) == X_LEG_REAIM | X_SYM_ROWS


def compile_key(lib, key, out_path=None, names=KEY23):
    k = (ctypes.c_int32 * len(names))(*[key.get(n, 0) for n in names])
    opts, log, ms = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(1 << 16), ctypes.c_double(0)
    rc = lib.sf_debug_wave_spec_compile(k, len(names), b"gfx950", None if out_path is None else str(out_path).encode(), opts, len(opts), log, len(log), ctypes.byref(ms))
    return rc, opts.value.decode().split("\n")[:-1], log.value.decode(errors="replace"), ms.value


def test_key_validity(lib):
    base = dict(BENCH_DEFAULT, **BENCH_FACTS)
    for mat_sym, index_x, ok in ((0, 0, True), (1, 0, True), (0, X_LEG_REAIM, True), (1, X_LEG_REAIM, True), (1, X_SYM_ROWS, True), (1, X_SYM_ROWS | X_LEG_REAIM, True),
                                 (0, X_SYM_ROWS, False), (0, X_SYM_ROWS | X_LEG_REAIM, False), (2, 0, False), (-1, X_SYM_ROWS, False), (1, 2048, False)):
        rc = compile_key(lib, dict(base, mat_sym=mat_sym, index_x=BENCH_INDEX | index_x))[0]
        assert rc == (R_NONE if ok else SF_ERR_INVALID), (mat_sym, index_x)
    # a key of 22 words names a matrix nobody has looked at: the bit that rests on the fact is refused, the other is not
    assert compile_key(lib, dict(base, index_x=X_SYM_ROWS), names=KEY22)[0] == SF_ERR_INVALID
    assert compile_key(lib, dict(base, index_x=X_LEG_REAIM), names=KEY22)[0] == R_NONE


WANT = {X_SYM_ROWS: ["-DSF_SPEC_SYM_ROWS=(1)"], X_LEG_REAIM: ["-DSF_SPEC_LEG_REAIM=(1)"]}


def test_options_of_the_candidates(lib):
    """Each candidate behind its own bit, after the index's; the fact alone adds nothing."""
    for mask in (0, X_SYM_ROWS, X_LEG_REAIM, X_SYM_ROWS | X_LEG_REAIM):
        rc, opts, _, _ = compile_key(lib, dict(BENCH_KEY, **BENCH_FACTS, mat_sym=1, index_x=mask))
        assert rc == R_NONE
        assert [o for o in opts if o.startswith("-D")][7:] == [o for bit in (X_SYM_ROWS, X_LEG_REAIM) if mask & bit for o in WANT[bit]], mask
    rc, opts, _, _ = compile_key(lib, dict(BENCH_DEFAULT, **BENCH_FACTS, mat_sym=1, index_x=BENCH_INDEX | X_SYM_ROWS | X_LEG_REAIM))
    assert rc == R_NONE and opts[-3:] == ["-DSF_SPEC_ROWS_FULL=(1)"] + WANT[X_SYM_ROWS] + WANT[X_LEG_REAIM]


# ---- the unit -----------------------------------------------------------------------------------------------------------------------------------
UNITS = {
    "sym_rows": dict(BENCH_DEFAULT, **BENCH_FACTS, mat_sym=1, index_x=BENCH_INDEX | X_SYM_ROWS),
    "leg_reaim": dict(BENCH_DEFAULT, **BENCH_FACTS, mat_sym=1, index_x=BENCH_INDEX | X_LEG_REAIM),
    "both": dict(BENCH_DEFAULT, **BENCH_FACTS, mat_sym=1, index_x=BENCH_INDEX | X_SYM_ROWS | X_LEG_REAIM),
    "leg_reaim_asymmetric_matrix": dict(BENCH_DEFAULT, **BENCH_FACTS, mat_sym=0, index_x=BENCH_INDEX | X_LEG_REAIM),
    "both_on_the_floor": dict(BENCH_KEY, **BENCH_FACTS, mat_sym=1, index_x=X_SYM_ROWS | X_LEG_REAIM),
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
