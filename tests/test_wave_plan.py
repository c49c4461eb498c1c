"""CPU tests of the wave engine's launch plan and engine resolution (csrc/sf_wave_plan.h: plan_wave_launch, wave_engine_fits,
wave_engine_default) through the diagnostic export sf_debug_wave_plan: no device, no context, every switch passed explicitly.  A golden
sweep recorded from the decision code this header replaced (tests/golden/wave_plan_sweep.json), the named sizes DESIGN and bench.py speak
of, and invariants of every accepted plan."""
import ctypes
import json
import os

import pytest

MAX_LEAVES = 2
# the int32 fields of WaveShape / WaveKnobs / WavePlan in declaration order (sf_wave_plan.h); the export refuses other counts
SHAPE = ["nbr_index", "V", "n_cap", "dim", "max_nearby", "levels", "mat32", "mat16", "small", "dist_level", "acceptor", "forager", "order", "dry_run",
         "n_leaves"] + ["kind%d" % i for i in range(MAX_LEAVES)] + ["n_replicas", "trace"]
KNOBS = ["no_compact", "max_wpe", "wpb_max", "node_global"]
PLAN = ["err", "levels", "mode", "compact", "wpe", "nodeg", "slice", "wpb", "grid", "block", "lds", "resident"]
SF_ERR_INVALID, SF_ERR_UNSUPPORTED = -1, -4
BUDGET = 160 * 1024 - 1024  # SF_LDS_BUDGET
REFUSAL = "wave engine cannot run this model (needs a nearby matrix meter, <= 65535 elements, LDS slice <= 160 KiB)"
NEARBY_CHANGE, NEARBY_SWAP = 16, 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_plan_sweep.json")


@pytest.fixture(scope="module")
def plan():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    fn = ctypes.CDLL(_lib.LIB_PATH).sf_debug_wave_plan
    fn.restype = ctypes.c_int32

    def run(shape, **knobs):
        k = dict(no_compact=0, max_wpe=6, wpb_max=4, node_global=-1)  # what wave_knobs() reads from an empty environment
        assert set(knobs) <= set(KNOBS) and set(shape) <= set(SHAPE), (knobs, shape)
        k.update(knobs)
        s = (ctypes.c_int32 * len(SHAPE))(*[shape.get(name, 0) for name in SHAPE])
        kk = (ctypes.c_int32 * len(KNOBS))(*[k[name] for name in KNOBS])
        out = (ctypes.c_int32 * len(PLAN))()
        msg = ctypes.c_char_p()
        fits = (ctypes.c_int32 * 2)()
        rc = fn(s, len(SHAPE), kk, len(KNOBS), out, len(PLAN), ctypes.byref(msg), fits)
        got = dict(zip(PLAN, out))
        assert rc == got["err"] and rc in (0, SF_ERR_UNSUPPORTED), rc
        assert (msg.value is None) == (rc == 0) and (rc == 0) == bool(fits[0])  # a launch is refused exactly when the engine cannot run the model
        assert msg.value is None or msg.value.decode() == REFUSAL
        got.update(fits=fits[0], default=fits[1])
        return got

    run.fn = fn
    return run


def cvrp(V, n, **kw):
    """A CVRP-shaped list class (n customers on V routes, one depot node more) under the default policy's two nearby leaves with the
    default components: u32 and u16 matrix copies, 32-bit trial arithmetic -- FAST + SMALL."""
    d = dict(nbr_index=1, V=V, n_cap=n, dim=n + 1, max_nearby=20, levels=2, mat32=1, mat16=1, small=1, dist_level=1, acceptor=1, forager=0, order=3,
             n_leaves=2, kind0=NEARBY_CHANGE, kind1=NEARBY_SWAP, n_replicas=1024)
    d.update(kw)
    return d


def key(got, *names):
    return tuple(got[n] for n in names)


# ---- the decisions of the code before plan_wave_launch ------------------------------------------------------------------------------------------
def test_golden_sweep(plan):
    """640 seeded rows; each expected decision was printed by the previous commit's launch_list_wave_t / wave_engine_possible /
    use_wave_engine, compiled verbatim into a host program (the file's own comment).  The sweep reaches every mode, both causes of a
    refusal, both sides of the default-engine rule and every switch value."""
    doc = json.load(open(GOLDEN))
    names = doc["shape"] + doc["knobs"] + doc["result"]
    modes, refused, seen, wrong = set(), set(), set(), []
    for values in doc["rows"]:
        row = dict(zip(names, values))
        got = plan(dict({n: row[n] for n in doc["shape"]}, nbr_index=1), **{n: row[n] for n in doc["knobs"]})
        if got["err"]:
            got.update(mode=-1)
            refused.add("range" if row["dim"] > 16384 or row["n_cap"] + row["V"] > 65535 else "slice")
        if any(got[n] != row[n] for n in doc["result"]):
            wrong.append((row, key(got, *doc["result"])))
        modes.add(row["mode"])
        if row["mode"] >= 0:
            seen.add(("combination", row["mat32"], row["mat16"], row["small"], row["mode"] >= 1, row["trace"]))
        seen.update({("wpb_max", row["wpb_max"]), ("no_compact", row["no_compact"]), ("max_wpe", row["max_wpe"]), ("node_global", row["node_global"]),
                     ("max_nearby", row["max_nearby"]), ("fits, default", row["fits"], row["default"])})
    assert not wrong, (len(wrong), wrong[:3])
    assert modes == {-1, 0, 1, 2, 3, 4, 5, 6} and refused == {"range", "slice"}
    want = {("wpb_max", v) for v in (1, 2, 3, 4)} | {("no_compact", v) for v in (0, 1)} | {("max_wpe", v) for v in (0, 4, 5, 6, 7)}
    want |= {("node_global", v) for v in (-1, 0, 1)} | {("max_nearby", v) for v in (1, 20, 32, 33, 64)} | {("fits, default", *v) for v in ((0, 0), (1, 0), (1, 1))}
    # FAST needs the u32 matrix and no trace; under those every combination of the others occurs, FAST or not
    want |= {("combination", m32, m16, sm, False, tr) for m32 in (0, 1) for m16 in (0, 1) for sm in (0, 1) for tr in (0, 1)}
    want |= {("combination", 1, m16, sm, True, 0) for m16 in (0, 1) for sm in (0, 1)}
    assert want <= seen, want - seen
    assert 300 <= len(doc["rows"]) and os.path.getsize(GOLDEN) < 64 * 1024


def test_invariants_of_accepted_plans(plan):
    doc = json.load(open(GOLDEN))
    names = doc["shape"] + doc["knobs"] + doc["result"]
    accepted = 0
    for values in doc["rows"]:
        row = dict(zip(names, values))
        got = plan(dict({n: row[n] for n in doc["shape"]}, nbr_index=1), **{n: row[n] for n in doc["knobs"]})
        if got["err"]:
            assert key(got, "mode", "slice", "wpb", "grid", "block", "lds", "resident") == (0,) * 7  # nothing is decided
            continue
        accepted += 1
        assert got["lds"] == got["slice"] * got["wpb"] <= BUDGET and got["block"] == 64 * got["wpb"], (row, got)
        assert got["grid"] == -(-row["n_replicas"] // got["wpb"]) and 1 <= got["wpb"] <= row["wpb_max"]
        assert got["levels"] == (2 if row["levels"] <= 2 else 4)
        assert 1 <= got["resident"] <= {4: 20, 5: 24}.get(got["mode"], 16) and got["resident"] % got["wpb"] == 0
        assert got["wpe"] == {4: 5, 5: 6}.get(got["mode"], 4)
        assert got["nodeg"] == (got["mode"] == 6) and got["compact"] == (got["mode"] >= 3)
        if got["compact"]:
            assert row["small"] and row["mat16"] and row["mat32"] and not row["trace"] and not row["no_compact"] and 1 <= row["V"] <= 1022
            assert row["node_global"] != 0 or not got["nodeg"]
            assert row["node_global"] != 1 or got["nodeg"]
    assert accepted >= 300


# ---- named sizes ----------------------------------------------------------------------------------------------------------------------------------
def test_cvrp_1000(plan):
    c = cvrp(100, 1000)
    assert key(plan(c), "mode", "resident", "wpb", "lds", "compact", "wpe", "nodeg") == (5, 24, 4, 26624, 1, 6, 0)
    for wpe in (6, 7):
        assert key(plan(c, max_wpe=wpe), "mode", "resident") == (5, 24)
    assert key(plan(c, max_wpe=5), "mode", "resident", "wpe") == (4, 20, 5)
    for knobs in (dict(max_wpe=4), dict(max_wpe=0), dict(no_compact=1)):
        assert key(plan(c, **knobs), "mode", "resident", "lds", "compact") == (2, 16, 37824, 0), knobs
    assert key(plan(c, node_global=1), "mode", "resident", "lds", "compact", "wpe", "nodeg") == (6, 16, 14528, 1, 4, 1)
    assert plan(c, node_global=0)["mode"] == 5
    for change in (dict(trace=1), dict(acceptor=0), dict(forager=2), dict(order=0), dict(dry_run=1), dict(dist_level=-1), dict(mat32=0),
                   dict(n_leaves=1), dict(kind0=NEARBY_SWAP, kind1=NEARBY_CHANGE)):
        assert plan(dict(c, **change))["mode"] == 0, change
    assert plan(dict(c, small=0))["mode"] == 1 and plan(dict(c, mat16=0))["mode"] == 2
    for wpb in (1, 2, 3):
        assert key(plan(c, wpb_max=wpb), "mode", "resident", "wpb", "lds", "block", "grid") == (5, 24, wpb, 6656 * wpb, 64 * wpb, -(-1024 // wpb))
    for levels, L in ((1, 2), (2, 2), (3, 4), (4, 4)):
        assert plan(dict(c, levels=levels))["levels"] == L


def test_cvrp_5000(plan):
    c = cvrp(500, 5000)
    assert key(plan(c), "mode", "resident", "wpb", "lds") == (6, 11, 1, 14032)  # bench.py: "11 per CU: launch mode 6"
    assert key(plan(c, node_global=0), "mode", "resident", "lds") == (3, 5, 29056)
    assert key(plan(c, no_compact=1), "mode", "resident", "slice", "wpb") == (2, 3, 43056, 3)


def test_mode_3_as_the_gpu_tests_reach_it(plan):
    assert plan(cvrp(150, 1500), max_wpe=4)["mode"] == 3 and key(plan(cvrp(150, 1500)), "mode", "resident") == (4, 17)


def test_first_sizes_of_the_default_ladder(plan):
    """n customers on n // 10 routes: 24 resident replicas per CU up to n = 1,031, mode 5 while more than 20 fit, mode 4 while more than
    16 do, then the COMPACT slice at 16 (mode 3) only until the table in HBM holds more."""
    first = {}
    for n in range(10, 1800):
        first.setdefault(plan(cvrp(n // 10, n))["mode"], n)
    assert first == {5: 10, 4: 1208, 3: 1530, 6: 1641}
    assert key(plan(cvrp(103, 1031)), "mode", "resident") == (5, 24) and key(plan(cvrp(103, 1032)), "mode", "resident") == (5, 23)


def test_mode_6_is_reached_through_mode_3_only(plan):
    """Behaviour as it stands (DESIGN, "Wave launch plan"): the node -> slot table goes to HBM only after a COMPACT mode was taken.  In a band
    near 958 routes x 10 the COMPACT slice holds no more replicas than the wide one (2 per CU), so the launch keeps mode 2 although the
    node-global slice would hold 6 -- whatever SF_AMD_NODE_GLOBAL says.  Beyond 1,022 routes the compact table cannot name a route."""
    band = cvrp(958, 9580)
    for knobs in (dict(), dict(node_global=1), dict(no_compact=1)):
        assert key(plan(band, **knobs), "mode", "resident", "wpb", "lds") == (2, 2, 1, 81536), knobs
    assert key(plan(cvrp(940, 9400)), "mode", "resident") == (6, 6) and key(plan(cvrp(963, 9630)), "mode", "resident") == (6, 6)
    assert key(plan(cvrp(1022, 10220)), "mode", "resident", "lds") == (6, 5, 27616)
    assert key(plan(cvrp(1023, 10230)), "mode", "resident", "lds") == (2, 1, 86992)
    assert plan(cvrp(1023, 10230), node_global=1)["mode"] == 2


# ---- engine resolution and refusals ----------------------------------------------------------------------------------------------------------------
def test_engine_resolution_edges(plan):
    ok = cvrp(100, 1000)
    assert key(plan(ok), "err", "fits", "default") == (0, 1, 1)
    for change, fits in ((dict(dim=16384), 1), (dict(dim=16385), 0), (dict(n_cap=65435), 1), (dict(n_cap=65436), 0), (dict(max_nearby=64), 1),
                         (dict(max_nearby=65), 0), (dict(nbr_index=0), 0)):
        got = plan(dict(ok, **change))
        assert key(got, "err", "fits") == (0 if fits else SF_ERR_UNSUPPORTED, fits), change
        assert fits or not got["default"]
    # the wide slice against the budget and against half of it (16-byte steps: 8 elements)
    slice_of = lambda n: plan(cvrp(100, n, dim=16384), no_compact=1)["slice"]
    n_half = max(n for n in range(1000, 20000, 8) if slice_of(n) <= BUDGET // 2)
    a, b = plan(cvrp(100, n_half, dim=16384), no_compact=1), plan(cvrp(100, n_half + 8, dim=16384), no_compact=1)
    assert (a["slice"], b["slice"]) == (BUDGET // 2, BUDGET // 2 + 16) and key(a, "fits", "default") == (1, 1) and key(b, "fits", "default") == (1, 0)
    n_full = n_half + (BUDGET - BUDGET // 2) // 2
    a, b = plan(cvrp(100, n_full, dim=16384), no_compact=1), plan(cvrp(100, n_full + 8, dim=16384), no_compact=1)
    assert key(a, "err", "slice", "resident", "wpb") == (0, BUDGET, 1, 1) and key(b, "err", "fits", "default") == (SF_ERR_UNSUPPORTED, 0, 0)


def test_export_refuses_other_counts(plan):
    s, k, out = (ctypes.c_int32 * len(SHAPE))(), (ctypes.c_int32 * len(KNOBS))(), (ctypes.c_int32 * len(PLAN))()
    assert plan.fn(s, len(SHAPE) - 1, k, len(KNOBS), out, len(PLAN), None, None) == SF_ERR_INVALID
    assert plan.fn(s, len(SHAPE), k, len(KNOBS) + 1, out, len(PLAN), None, None) == SF_ERR_INVALID
    assert plan.fn(s, len(SHAPE), k, len(KNOBS), out, len(PLAN) + 1, None, None) == SF_ERR_INVALID
