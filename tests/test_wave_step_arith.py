"""CPU tests of the 32-bit Barrett index the wave engine's COMPACT kernels fill their entity order tables with (csrc/sf_common.h:
perm_index_recip / mod_u32_recip), through the diagnostic export sf_debug_step_arith: no device, no context.  The index must equal
fastmod_u64 -- the form it replaces -- and (start + k x stride) mod V itself, for every list count V the COMPACT layout admits (2 .. 1,022),
every (start, stride, k) on the edges of their ranges, every k of a seeded (start, stride), and, beyond what the kernel needs, any 32-bit
argument.  (The remainder helpers of the levers that were measured and not kept, and their tests, are in profiles/wave_step_levers.patch.)"""
import ctypes

import numpy as np
import pytest

SF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def arith():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    fn = ctypes.CDLL(_lib.LIB_PATH).sf_debug_step_arith
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]

    def run(what, start, stride, V, ks):
        ks = np.ascontiguousarray(ks, dtype=np.uint32)
        out = np.empty(len(ks), dtype=np.uint32)
        rc = fn(what, start, stride, V, ks.ctypes.data, len(ks), out.ctypes.data)
        assert rc == 0, (rc, what, start, stride, V)
        return out

    run.fn = fn
    return run


def _edges(V, lowest=0):
    return sorted({0, 1, 2, V // 2, V - 2, V - 1} & set(range(lowest, V)))


def test_barrett_table_index_equals_fastmod(arith):
    """(start + k x stride) mod V: the 32-bit Barrett step against the 64 x 64 high multiply it replaces, every V the COMPACT layout admits.
    start and k run over 0 .. V - 1, a stride over 1 .. V - 1."""
    rng = np.random.default_rng(21)
    for V in range(2, 1023):
        ks = np.array(_edges(V), dtype=np.uint32)
        for start in _edges(V):
            for stride in _edges(V, 1):
                got, ref = arith(0, start, stride, V, ks), arith(1, start, stride, V, ks)
                assert (got == ref).all(), (V, start, stride)
                assert (got == (start + ks.astype(np.uint64) * stride) % V).all(), (V, start, stride)
        # a seeded (start, stride), every k: a stride coprime to V visits every list exactly once
        start, stride = int(rng.integers(0, V)), int(rng.integers(1, V))
        ks = np.arange(V, dtype=np.uint32)
        got = arith(0, start, stride, V, ks)
        assert (got == arith(1, start, stride, V, ks)).all(), (V, start, stride)
        if np.gcd(stride, V) == 1:
            assert sorted(got.tolist()) == list(range(V)), (V, start, stride)


def test_barrett_table_index_any_32_bit_argument(arith):
    """The step is exact for any 32-bit argument, not only below 2^21: start at the top of the range, k = 0."""
    for V in (2, 3, 127, 128, 1021, 1022):
        for x in (0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, (1 << 21) - 1, 1 << 21):
            assert arith(0, x, 1, V, [0])[0] == x % V, (V, x)


def test_export_refuses_what_the_helper_does_not_cover(arith):
    k = np.zeros(1, dtype=np.uint32)
    out = np.zeros(1, dtype=np.uint32)
    for what, V in [(0, 0), (0, 1), (0, 1023), (1, 1), (2, 2), (-1, 2)]:
        assert arith.fn(what, 0, 1, V, k.ctypes.data, 1, out.ctypes.data) == SF_ERR_INVALID
    assert arith.fn(0, 0, 1, 2, None, 1, out.ctypes.data) == SF_ERR_INVALID
