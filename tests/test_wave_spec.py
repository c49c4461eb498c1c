"""CPU tests of the wave engine's run-time specialisation (csrc/sf_wave_spec.h): the policy wave_spec_wanted on both sides of each gate
(sf_debug_wave_spec_gate), the compiler's option list for a key, and the device-only unit csrc/sf_tu_list_wave_spec.hip compiled for gfx950
through hiprtc without a device (sf_debug_wave_spec_compile) for one two-level and one four-level key, with the notes of the resulting code
object read back: one kernel, no scratch."""
import ctypes
import os
import re
import subprocess

import pytest

GATE = ["mode", "move_budget", "n_steps", "n_replicas", "resident", "cus", "knob"]  # WaveSpecGate, declaration order
KEY = ["levels", "wpe", "V", "dim", "n_cap", "k0", "k1", "extras", "capacity", "cap_weight", "dist_weight", "depot", "cap_level", "dist_level", "la_size", "limit",
       "has_perm", "has_explicit"]  # WaveSpecKey
X_MODEL, X_LA, X_LIMIT, X_PERM, X_EXPLICIT = 1, 2, 4, 8, 16
R_NONE, R_KNOB, R_MODE, R_BUDGET, R_STEPS, R_RESIDENCY = 0, 1, 2, 3, 4, 5
R_NO_HIPRTC, R_NO_SOURCES, R_COMPILE = 10, 11, 12
SF_ERR_INVALID = -1
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
# the timed leg of bench.py: CVRP-1000 / 100 vehicles, max_nearby 20, launch mode 5, 98,304 replicas on 256 CUs of 24
BENCH_KEY = dict(levels=2, wpe=6, V=100, dim=1001, n_cap=1000, k0=20, k1=20)
BENCH_GATE = dict(mode=5, move_budget=0, n_steps=100, n_replicas=98304, resident=24, cus=256, knob=-1)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    L.sf_debug_wave_spec_gate.restype = ctypes.c_int32
    L.sf_debug_wave_spec_compile.restype = ctypes.c_int32
    L.sf_debug_wave_spec.restype = ctypes.c_int32
    return L


def gate(lib, **kw):
    g = dict(BENCH_GATE)
    assert set(kw) <= set(GATE)
    g.update(kw)
    return lib.sf_debug_wave_spec_gate((ctypes.c_int32 * len(GATE))(*[g[n] for n in GATE]), len(GATE))


def compile_key(lib, key, out_path=None, arch=b"gfx950"):
    k = (ctypes.c_int32 * len(KEY))(*[key.get(n, 0) for n in KEY])
    opts, log, ms = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(1 << 16), ctypes.c_double(0)
    rc = lib.sf_debug_wave_spec_compile(k, len(KEY), arch, None if out_path is None else str(out_path).encode(), opts, len(opts), log, len(log), ctypes.byref(ms))
    return rc, opts.value.decode().split("\n")[:-1], log.value.decode(errors="replace"), ms.value


# ---- the policy ---------------------------------------------------------------------------------------------------------------------------------
def test_the_benchmark_launch_is_specialised(lib):
    assert gate(lib) == R_NONE


@pytest.mark.parametrize("mode,want", [(0, R_MODE), (1, R_MODE), (2, R_MODE), (3, R_NONE), (4, R_NONE), (5, R_NONE), (6, R_MODE)])
def test_gate_mode(lib, mode, want):
    """Launch modes 3, 4 and 5 only, whatever the switch says."""
    assert gate(lib, mode=mode) == want
    assert gate(lib, mode=mode, knob=1) == want
    assert gate(lib, mode=mode, knob=0) == R_KNOB


def test_gate_move_budget(lib):
    assert gate(lib, move_budget=0) == R_NONE and gate(lib, move_budget=1) == R_BUDGET


def test_gate_steps(lib):
    assert gate(lib, n_steps=49) == R_STEPS and gate(lib, n_steps=50) == R_NONE


def test_gate_residency(lib):
    """At least one full residency, equality included (bench.py's counter children run exactly one)."""
    full = 24 * 256
    assert gate(lib, n_replicas=full - 1) == R_RESIDENCY and gate(lib, n_replicas=full) == R_NONE
    assert gate(lib, n_replicas=1024) == R_RESIDENCY  # the tuned leg of the benchmark keeps the ahead-of-time kernel
    assert gate(lib, n_replicas=5120, resident=20) == R_NONE and gate(lib, n_replicas=5119, resident=20) == R_RESIDENCY


def test_gate_switch(lib):
    """SF_AMD_WAVE_SPEC=0 never; =1 whenever the mode allows -- short launches, budgets and small launches included; unset: the rule."""
    assert gate(lib, knob=0) == R_KNOB
    assert gate(lib, knob=1, n_steps=1, move_budget=1, n_replicas=1) == R_NONE
    assert gate(lib, knob=-1, n_steps=1) == R_STEPS


def test_gate_refuses_other_sizes(lib):
    assert lib.sf_debug_wave_spec_gate((ctypes.c_int32 * 3)(), 3) == SF_ERR_INVALID
    assert lib.sf_debug_wave_spec(None, (ctypes.c_int32 * 3)(), 3) == SF_ERR_INVALID


# ---- the option list ----------------------------------------------------------------------------------------------------------------------------
def test_options_for_a_key(lib):
    rc, opts, _, _ = compile_key(lib, BENCH_KEY)
    assert rc == R_NONE
    from solverforge_amd import _lib

    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "csrc")
    assert opts[:5] == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + csrc]  # the Makefile's flags, the sources beside the library
    defs = [o for o in opts if o.startswith("-D")]
    assert defs == ["-DSF_SPEC_L=2", "-DSF_SPEC_WPE=6", "-DSF_SPEC_V(x)=100", "-DSF_SPEC_DIM(x)=1001", "-DSF_SPEC_NCAP(x)=1000", "-DSF_SPEC_K0(x)=20", "-DSF_SPEC_K1(x)=20"]
    assert all(o.startswith(("-I", "-D")) for o in opts[4:])
    rc, opts4, _, _ = compile_key(lib, dict(BENCH_KEY, levels=4, wpe=4, k1=33))
    assert rc == R_NONE and "-DSF_SPEC_L=4" in opts4 and "-DSF_SPEC_WPE=4" in opts4 and "-DSF_SPEC_K1(x)=33" in opts4


def test_options_of_the_candidates(lib):
    """Each candidate behind its own switch: nothing of one that is off reaches the compiler."""
    full = dict(BENCH_KEY, capacity=55, cap_weight=1, dist_weight=1, depot=7, cap_level=0, dist_level=1, la_size=400, limit=256, has_perm=1, has_explicit=0)
    want = {X_MODEL: ["-DSF_SPEC_MODEL_WORDS=(1)", "-DSF_SPEC_CAPACITY=(55)", "-DSF_SPEC_CAP_WEIGHT=(1)", "-DSF_SPEC_DIST_WEIGHT=(1)", "-DSF_SPEC_DEPOT=(7)", "-DSF_SPEC_CAP_LEVEL=(0)",
                      "-DSF_SPEC_DIST_LEVEL=(1)"],
            X_LA: ["-DSF_SPEC_LA_SIZE(x)=400"], X_LIMIT: ["-DSF_SPEC_LIMIT(x)=256"], X_PERM: ["-DSF_SPEC_HAS_PERM(x)=1"], X_EXPLICIT: ["-DSF_SPEC_HAS_EXPLICIT(x)=0"]}
    for mask in (0, X_MODEL, X_LA, X_LIMIT, X_PERM, X_EXPLICIT, 31):
        rc, opts, _, _ = compile_key(lib, dict(full, extras=mask))
        assert rc == R_NONE
        extra = [o for o in opts if o.startswith("-D")][7:]
        assert extra == [o for bit in (X_MODEL, X_LA, X_LIMIT, X_PERM, X_EXPLICIT) if mask & bit for o in want[bit]], mask


def test_bad_keys_are_refused(lib):
    for bad in (dict(levels=3), dict(wpe=7), dict(V=0), dict(k0=0), dict(extras=32), dict(extras=X_LA, la_size=0), dict(extras=X_LIMIT, limit=0)):
        assert compile_key(lib, dict(BENCH_KEY, **bad))[0] == SF_ERR_INVALID


# ---- the unit, compiled in process for gfx950 without a device ----------------------------------------------------------------------------------
def kernel_notes(path):
    """The amdhsa.kernels entries of a code object: [(name, {field: int})]."""
    txt = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = []
    for line in txt.split("\n"):
        if line.startswith("  - ."):
            out.append({})
            line = "    " + line[4:]
        m = re.match(r"^    (\.[a-z_]+):\s+(.*)$", line)
        if m and out:
            out[-1][m.group(1)] = m.group(2).strip("'\"")
    return [k for k in out if ".name" in k and ".vgpr_count" in k]


ALL_CANDIDATES = dict(extras=31, capacity=55, cap_weight=1, dist_weight=1, depot=0, cap_level=0, dist_level=1, la_size=400, limit=256, has_perm=1, has_explicit=0)


@pytest.mark.parametrize("key", [BENCH_KEY, dict(levels=4, wpe=5, V=8, dim=41, n_cap=40, k0=20, k1=20), dict(BENCH_KEY, **ALL_CANDIDATES)],
                         ids=["two_level_bench", "four_level", "two_level_bench_all_candidates"])
def test_unit_compiles_without_a_device(lib, tmp_path, key):
    co = tmp_path / "spec.co"
    rc, _, log, ms = compile_key(lib, key, co)
    assert rc == R_NONE, log[-4000:]
    print("compile ms", round(ms))
    ks = kernel_notes(co)
    assert len(ks) == 1, [k[".name"] for k in ks]  # exactly one kernel
    k = ks[0]
    assert "k_list_search_wave" in k[".name"]  # bench.py's counter passes and kernel-time record select by this substring
    print({f: k[f] for f in (".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size")})
    assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".vgpr_spill_count"]) == 0  # no scratch
    assert int(k[".vgpr_count"]) <= 512 // key["wpe"]  # the waves per SIMD it was compiled for
    assert int(k[".max_flat_workgroup_size"]) == 256


def test_missing_sources_are_a_reason_not_an_error(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("SF_AMD_CSRC", str(tmp_path))
    rc, opts, _, _ = compile_key(lib, BENCH_KEY, tmp_path / "none.co")
    assert rc in (R_NO_SOURCES, R_NO_HIPRTC) and "-I" + str(tmp_path) in opts
    assert not (tmp_path / "none.co").exists()
