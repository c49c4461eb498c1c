"""CPU: the LimitedNeighborhood entry points are declared in include/solverforge_amd.h, listed in _lib.SYMBOLS, exported by the library and
wrapped by the director; the header says what they promise (no compute calls: no GPU needed)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_selector_limit", "sf_union_limit", "sf_vnd_set_neighborhoods")


def _header():
    return open(os.path.join(ROOT, "include", "solverforge_amd.h")).read()


def test_symbols_are_declared_listed_and_exported():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    header = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("LimitedNeighborhood",):
        assert name in integration, name


def test_declarations_and_header_text():
    header = " ".join(re.sub(r"^ \* ", " ", _header(), flags=re.M).split())  # (comment continuation lines start with " * ")
    assert "int32_t sf_selector_limit(sf_ctx* ctx, int32_t leaf_index, int64_t selected_count_limit);" in header
    assert "int32_t sf_union_limit(sf_ctx* ctx, int64_t selected_count_limit);" in header
    assert ("int32_t sf_vnd_set_neighborhoods(sf_ctx* ctx, int32_t n_hoods, const int32_t* first_leaf, const int32_t* union_order, "
            "const int64_t* hood_limit);") in header
    for phrase in ("limited.rs:14-94", "-1 removes it", "stored as none", "takes effect at the next launch", "its own child count",
                   "n_hoods == 0 returns to one leaf each", "Takes effect at the next sf_phase_start", "list ruin, scalar ruin or critical-path leaf"):
        assert phrase in header, phrase


def test_argument_checks_need_no_device():
    """The value rules of the three calls are checked before anything touches the device: a context that was never initialised answers."""
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    L = _lib.load()
    assert L.sf_selector_limit(None, 0, 1) != 0 and L.sf_union_limit(None, 1) != 0 and L.sf_vnd_set_neighborhoods(None, 0, None, None, None) != 0


def test_director_wraps_them():
    import solverforge_amd as sfa

    for name in ("limit_selector", "limit_union", "set_vnd_neighborhoods"):
        assert callable(getattr(sfa.GpuScoreDirector, name)), name
    assert list(inspect.signature(sfa.GpuScoreDirector.limit_selector).parameters)[1:] == ["leaf", "selected_count_limit"]
    assert list(inspect.signature(sfa.GpuScoreDirector.limit_union).parameters)[1:] == ["selected_count_limit"]
    assert list(inspect.signature(sfa.GpuScoreDirector.set_vnd_neighborhoods).parameters)[1:] == ["groups", "union_orders", "limits"]
