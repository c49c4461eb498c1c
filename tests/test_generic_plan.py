"""CPU tests of the generic engine's launch plan (csrc/sf_mixed_plan.h: plan_generic_launch) through the diagnostic export
sf_debug_generic_plan: no device, no context, every switch passed explicitly.  The documented edge sizes of every placement gate of a
precedence model (the table in test_gpu_prec_placement.py's docstring), the MODE 2 gate and the workgroup shape behind it, the choice of
instantiation and ruin variant, the Python restatement of the rules the GPU tests rely on (prec_placement_rules.py) against the library,
and invariants of every accepted plan over a seeded sweep of shapes."""
import ctypes
import random

import pytest
from prec_placement_rules import default_trials, forced_trials, static_copy, trials

GL = 12
# the int32 fields of GenericShape / GenericKnobs / GenericPlan in declaration order (sf_mixed_plan.h); the export refuses other counts
SHAPE = (["has_list", "has_scalar", "n_scalar", "n_values", "tables", "run_level", "run_P", "V", "n_cap", "dim", "leg16", "small32", "mat16",
          "mat_symmetric", "dist_level", "levels", "n_leaves"] + ["kind%d" % i for i in range(GL)] +
         ["has_nearby", "kopt_nearby", "has_ruin", "union_custom", "union_order", "acceptor", "forager", "order", "dry_run", "legacy_eval",
          "explicit_seeds", "prec_on", "prec_n", "prec_edges", "prec_owner", "plf_on", "n_replicas", "trace"])
KNOBS = ["no_fast", "no_pre_eval", "prec_no_occ", "debug_launch", "wpb_max", "plf_slow", "plf_force64", "prec_hbm", "prec_lds_max_set",
         "prec_lds_max_kb", "prec_inc", "prec_static_hbm", "prec_no_slim", "prec_groups_set", "prec_groups", "prec_no_sweep"]
PLAN = ["err", "levels", "value_bytes", "ruin_inst", "prec", "mode", "nodeg", "ring32", "ruin_variant", "prec_lds", "prec_static",
        "prec_static_slim", "prec_groups", "prec_sweep", "prec_inc", "slice", "wpb", "grid", "block", "lds", "resident", "flags"]
SF_ERR_UNSUPPORTED = -4
CU_LDS, BUDGET = 160 * 1024, 160 * 1024 - 1024
STATIC_LDS, PREC_STATIC_LDS = 1024, 1184  # SF_MIXED_STATIC_LDS / SF_MIXED_PREC_STATIC_LDS (sf_mixed_wave.hip); the FAST kernels hold none
LIST_CHANGE, LIST_SWAP, NEARBY_CHANGE, NEARBY_SWAP, REVERSE, SUB_CHANGE, SUB_SWAP, KOPT, RUIN, PERMUTE, PRECEDENCE = 4, 8, 16, 32, 64, 128, 256, 512, 1024, 8192, 16384


@pytest.fixture(scope="module")
def plan():
    import __graft_entry__ as g

    g.build()
    from solverforge_amd import _lib

    fn = ctypes.CDLL(_lib.LIB_PATH).sf_debug_generic_plan
    fn.restype = ctypes.c_int32

    def run(shape, **knobs):
        k = dict({name: 0 for name in KNOBS}, wpb_max=4)
        assert set(knobs) <= set(KNOBS) and set(shape) <= set(SHAPE), (knobs, shape)
        k.update(knobs)
        s = (ctypes.c_int32 * len(SHAPE))(*[shape.get(name, 0) for name in SHAPE])
        kk = (ctypes.c_int32 * len(KNOBS))(*[k[name] for name in KNOBS])
        out = (ctypes.c_int32 * len(PLAN))()
        msg = ctypes.c_char_p()
        rc = fn(s, len(SHAPE), kk, len(KNOBS), out, len(PLAN), ctypes.byref(msg))
        got = dict(zip(PLAN, out))
        assert rc == got["err"] and rc in (0, SF_ERR_UNSUPPORTED), rc
        assert (msg.value is None) == (rc == 0)
        got["msg"] = msg.value.decode() if msg.value else None
        got["static"] = 0 if not got["prec_static"] else (2 if got["prec_static_slim"] else 1)  # as sf_list_arith_flags reports the copy
        return got

    return run


def leaves(*kinds):
    d = {"n_leaves": len(kinds)}
    d.update({"kind%d" % i: k for i, k in enumerate(kinds)})
    d["has_ruin"] = int(RUIN in kinds)
    d["has_nearby"] = sum(k in (NEARBY_CHANGE, NEARBY_SWAP) for k in kinds)
    return d


def list_model(V, n_cap, dim=None, **kw):
    """A list class with a symmetric 16-bit matrix meter under the default components of a list slot (LateAcceptance + AcceptedCount, the
    default root union, random selection order) -- what the FAST instantiation asks for."""
    d = dict(has_list=1, V=V, n_cap=n_cap, dim=n_cap if dim is None else dim, leg16=1, small32=1, mat16=1, mat_symmetric=1, dist_level=1, levels=2,
             union_order=4, acceptor=1, forager=0, order=3, n_replicas=1)
    d.update(kw)
    return d


def prec_shape(n, V, E=None, owner=True, capacity=None, kinds=(LIST_CHANGE, LIST_SWAP), R=1, **kw):
    """List-only precedence model as build_precedence_shop declares it: n nodes on V lists, no distance / capacity constraint."""
    d = list_model(V, n if capacity is None else capacity, dim=n, leg16=0, small32=0, mat16=0, mat_symmetric=0, dist_level=-1, n_replicas=R)
    d.update(prec_on=1, prec_n=n, prec_edges=n // 2 if E is None else E, prec_owner=int(owner), forager=2)
    d.update(leaves(*kinds))
    d["plf_on"] = int(PRECEDENCE in kinds or RUIN in kinds)
    d.update(kw)
    return d


# ---- the documented edges of the placement gates -------------------------------------------------------------------------------------------
def test_kahn_scratch_edges(plan):
    a, b = plan(prec_shape(11493, 8)), plan(prec_shape(11494, 8))
    assert (a["err"], a["slice"], a["prec_lds"], a["prec_sweep"]) == (0, 161792, 1, 0)
    assert (b["err"], b["prec_lds"], b["prec_sweep"], b["static"], b["prec_groups"]) == (0, 0, 1, 0, 0)
    for n, lds in ((3072, 1), (3073, 0)):
        got = plan(prec_shape(n, 8, owner=False), prec_lds_max_set=1, prec_lds_max_kb=36)
        assert (got["prec_lds"], got["prec_sweep"]) == (lds, 1 - lds), n
        assert plan(prec_shape(n, 8, owner=False))["prec_lds"] == 1
    assert plan(prec_shape(3072, 8), prec_hbm=1)["prec_lds"] == 0
    # the sweep is the default of the HBM scratch only: not with the incremental refresh, the switch, or the critical-path leaf's tables
    assert plan(prec_shape(11494, 8), prec_inc=1)["prec_sweep"] == 0 and plan(prec_shape(11494, 8), prec_inc=1)["prec_inc"] == 1
    assert plan(prec_shape(11494, 8), prec_no_sweep=1)["prec_sweep"] == 0
    got = plan(prec_shape(11494, 8, plf_on=1), prec_inc=1)
    assert (got["prec_sweep"], got["prec_inc"]) == (0, 0)


@pytest.mark.parametrize("owner,n,E,static", [(True, 500, 295, 1), (True, 500, 296, 2), (False, 600, 245, 1), (False, 600, 246, 2)])
def test_full_copy_edges(plan, owner, n, E, static):
    got = plan(prec_shape(n, 12, E=E, owner=owner))
    assert got["static"] == static and got["prec_lds"] == 1
    assert got["prec_static"] == ((28 if owner else 24) * n + 8 * E + 24 if static == 1 else (16 if owner else 12) * n + 16)
    assert got["prec_groups"] == (default_trials(n, 12) if static == 1 else 0)
    assert plan(prec_shape(n, 12, E=E, owner=owner), prec_static_hbm=1)["static"] == 0
    assert plan(prec_shape(n, 12, E=E, owner=owner), prec_no_slim=1)["static"] == (1 if static == 1 else 0)


@pytest.mark.parametrize("owner,n,static", [(True, 2559, 2), (True, 2560, 0), (False, 3412, 2), (False, 3413, 0)])
def test_slim_copy_edges(plan, owner, n, static):
    got = plan(prec_shape(n, 8, owner=owner))
    assert (got["static"], got["prec_lds"], got["prec_groups"]) == (static, 1, 0)


def test_copy_fit_edges(plan):
    a, b = plan(prec_shape(3400, 8, owner=False, capacity=39648)), plan(prec_shape(3400, 8, owner=False, capacity=39649))
    assert (a["err"], a["slice"], a["static"], a["prec_static"]) == (0, 120976, 2, 40816)
    assert (b["err"], b["static"], b["prec_lds"]) == (0, 0, 1)


def test_groups_fit_edges(plan):
    a, b = plan(prec_shape(428, 5, capacity=63888)), plan(prec_shape(428, 5, capacity=63889))
    assert (a["err"], a["prec_groups"], a["static"], a["slice"]) == (0, 2, 1, 148064)
    assert (b["err"], b["prec_groups"], b["static"], b["slice"]) == (0, 0, 1, 133776)
    for capacity, T in ((57928, 8), (57929, 4), (65160, 4), (65161, 2)):
        got = plan(prec_shape(300, 3, capacity=capacity), prec_groups_set=1, prec_groups=16)
        assert (got["err"], got["prec_groups"], got["static"]) == (0, T, 1), capacity


def test_default_trials_edges(plan):
    assert [plan(prec_shape(n, 5))["prec_groups"] for n in (80, 81, 244, 245, 428, 429)] == [16, 8, 4, 2, 2, 0]


def test_python_rules_agree_with_the_library(plan):
    """prec_placement_rules.py (what the GPU tests compute their expected placements with) against the plan, on models whose slice is far
    from every whole-slice gate (element capacity = node count, at most 3,413 nodes)."""
    for n in (1, 2, 48, 80, 81, 244, 245, 300, 428, 429, 500, 585, 600, 682, 683, 1000, 2559, 2560, 3412, 3413):
        for V in (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 32, 33, 63, 64, 65):
            for E in sorted({0, n // 2, n - 1}):
                for owner in (False, True):
                    got = plan(prec_shape(n, V, E=E, owner=owner))
                    st = static_copy(n, E, owner)
                    assert (got["err"], got["prec_lds"]) == (0, 1)
                    assert got["static"] == st, (n, V, E, owner)
                    assert got["prec_groups"] == trials(n, V, st) == (default_trials(n, V) if st == 1 else 0), (n, V, E, owner)
                    assert plan(prec_shape(n, V, E=E, owner=owner), prec_no_slim=1)["static"] == static_copy(n, E, owner, slim=False)
                    for forced in (0, 2, 3, 4, 8, 16, 32):
                        got = plan(prec_shape(n, V, E=E, owner=owner), prec_groups_set=1, prec_groups=forced)
                        assert got["prec_groups"] == trials(n, V, st, forced) == (forced_trials(n, V, forced) if st == 1 else 0), (n, V, E, owner, forced)


# ---- MODE 2 ----------------------------------------------------------------------------------------------------------------------------------
def test_mode2_gate_and_workgroup_shape(plan):
    a, b = plan(prec_shape(1217, 8, R=2049)), plan(prec_shape(1218, 8, R=2049))
    assert (a["slice"], a["mode"]) == (17936, 2) and (b["slice"], b["mode"]) == (17952, 0)
    assert plan(prec_shape(1217, 8, R=2048))["mode"] == 0
    assert plan(prec_shape(1217, 8, R=2049, trace=1))["mode"] == 0
    assert plan(prec_shape(1217, 8, R=2049), prec_no_occ=1)["mode"] == 0
    # without owners: slim copy 14,620 bytes; a workgroup of w replicas takes 17,936 w + 1,184 + 14,620 bytes, so 4, 3, 2, 1 of them fit a
    # CU: 4, 6, 6, 4 resident replicas (at most 16 waves by registers); the tie goes to the larger group
    got = plan(prec_shape(1217, 8, R=2049, owner=False))
    assert (got["static"], got["prec_static"], got["mode"]) == (2, 14620, 2)
    assert [CU_LDS // (17936 * w + PREC_STATIC_LDS + 14620) * w for w in (1, 2, 3, 4)] == [4, 6, 6, 4]
    assert (got["wpb"], got["resident"], got["grid"], got["block"], got["lds"]) == (3, 6, 683, 192, 68428)
    capped = plan(prec_shape(1217, 8, R=2049, owner=False), wpb_max=2)
    assert (capped["wpb"], capped["resident"], capped["grid"], capped["block"], capped["lds"]) == (2, 6, 1025, 128, 2 * 17936 + 14620)


# ---- the instantiation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,L", [(1, 2), (2, 2), (3, 4), (4, 4)])
def test_value_bytes_and_level_template(plan, levels, L):
    for prec in (0, 1):
        for n_values, n_scalar, vb in ((127, 1024, 1), (128, 1024, 2), (127, 1023, 2), (2, 5000, 1)):
            s = prec_shape(1024, 128, owner=False) if prec else list_model(4, 100, **leaves(LIST_CHANGE, LIST_SWAP))
            s.update(has_scalar=1, n_scalar=n_scalar, n_values=n_values, levels=levels, n_leaves=4, kind2=1, kind3=2)
            got = plan(s)
            assert (got["err"], got["levels"], got["value_bytes"], got["ruin_inst"], got["prec"], got["mode"]) == (0, L, vb, 0, prec, 0)
            one, two = plan(dict(s, n_values=127)), plan(dict(s, n_values=128))
            a16 = lambda x: (x + 15) // 16 * 16  # the value array: one byte per entity instead of two
            assert two["slice"] - one["slice"] == (a16(2 * n_scalar) - a16(n_scalar) if n_scalar >= 1024 else 0)
    # a scalar-less model, and a ruin leaf (i16 instantiations only)
    assert plan(list_model(4, 100, levels=levels, **leaves(LIST_CHANGE, LIST_SWAP)))["value_bytes"] == 2
    s = list_model(4, 100, levels=levels, has_scalar=1, n_scalar=2048, n_values=3, **leaves(LIST_CHANGE, RUIN, 1, 2))
    got = plan(s)
    assert (got["levels"], got["value_bytes"], got["ruin_inst"], got["prec"]) == (L, 2, 1, 0)
    got = plan(prec_shape(200, 5, kinds=(LIST_CHANGE, RUIN), levels=levels, has_scalar=1, n_scalar=2048, n_values=3))
    assert (got["levels"], got["value_bytes"], got["ruin_inst"], got["prec"]) == (L, 2, 1, 1)


def test_fast_and_ruin_variant(plan):
    policy = (NEARBY_CHANGE, NEARBY_SWAP, SUB_CHANGE, SUB_SWAP, REVERSE, KOPT, RUIN)
    base = list_model(10, 1000, dim=1001, kopt_nearby=1, **leaves(*policy))
    got = plan(base)
    assert (got["err"], got["mode"], got["nodeg"], got["ring32"], got["ruin_variant"], got["ruin_inst"], got["value_bytes"]) == (0, 1, 1, 1, 3, 1, 2)
    assert got["wpb"] * got["slice"] == got["lds"]
    assert plan(base, no_pre_eval=1)["ring32"] == 0 and plan(dict(base, small32=0))["mode"] == 0
    # everything the FAST kernels compile out keeps the general instantiation; the list-preserving recreate stays (rv2_model_ok holds)
    general = [dict(trace=1), dict(acceptor=0), dict(forager=1), dict(dry_run=1), dict(union_custom=1), dict(union_order=3), dict(order=0),
               dict(mat_symmetric=0), dict(legacy_eval=1), dict(explicit_seeds=1), dict(kopt_nearby=0), dict(kind0=LIST_CHANGE),
               dict(has_scalar=1, n_scalar=10, n_values=4)]
    for change in general:
        got = plan(dict(base, **change))
        assert (got["err"], got["mode"], got["nodeg"], got["ring32"], got["ruin_variant"]) == (0, 0, 0, 0, 3), change
    assert plan(base, no_fast=1)["mode"] == 0
    assert plan(dict(base, mat_symmetric=0, dist_level=-1))["mode"] == 1  # no distance constraint: nothing asymmetric to price
    assert plan(dict(base, **leaves(NEARBY_CHANGE)))["mode"] == 0  # a single leaf is no union
    # with a ruin leaf FAST carries the list-preserving recreate only: leg16 and rv2_model_ok, at their edges
    # (no nearby leaves here: the general instantiation's node -> slot table of 32,768 nodes would not fit the slice)
    far = dict(base, **leaves(*policy[2:]))
    for change, variant in ((dict(leg16=0), 1), (dict(mat16=0), 2), (dict(small32=0), 2), (dict(V=129), 2), (dict(n_cap=32768), 2), (dict(dim=32768), 2)):
        got = plan(dict(far, **change))
        assert (got["err"], got["mode"], got["ruin_variant"]) == (0, 0, variant), change
    for change in (dict(), dict(V=128), dict(n_cap=32767), dict(dim=32767)):
        got = plan(dict(far, **change))
        assert (got["err"], got["mode"], got["ruin_variant"]) == (0, 1, 3), change
    # without the leaf those do not matter
    got = plan(dict(base, leg16=0, mat16=0, **leaves(*policy[:-1])))
    assert (got["mode"], got["nodeg"], got["ruin_variant"], got["ruin_inst"]) == (1, 1, 0, 0)
    # a small model, where registers alone bound the residents: four workgroups of four waves per CU, three with the ruin leaf
    small = list_model(4, 100, dim=101, kopt_nearby=1)
    assert plan(dict(small, **leaves(*policy[:-1])))["resident"] == 16 and plan(dict(small, **leaves(*policy)))["resident"] == 12
    assert plan(dict(small, **leaves(*policy)), no_fast=1)["resident"] == 8 and plan(prec_shape(100, 4, R=2049), prec_groups_set=1)["resident"] == 16


def test_refusals(plan):
    got = plan(prec_shape(100, 4, capacity=65535, kinds=(LIST_CHANGE, RUIN), dim=65536, leg16=1))
    assert (got["err"], got["msg"]) == (SF_ERR_UNSUPPORTED, "model does not fit one wave's LDS slice")
    # A slice inside the 159 KiB budget whose workgroup passes 160 KiB with the PREC kernels' static LDS beside it (HBM scratch: no whole-slice
    # test took a margin).  8 lists of capacity 60,000 beside x scalar entities of two bytes: 64 + 48 + 120,000 + a16(2 x) + 128 + 768.
    def mixed(x):
        return prec_shape(100, 8, capacity=60000, has_scalar=1, n_scalar=x, n_values=200)

    ok, over, budget = plan(mixed(20824), prec_hbm=1), plan(mixed(20825), prec_hbm=1), plan(mixed(20904), prec_hbm=1)
    assert (ok["err"], ok["slice"], ok["wpb"], ok["resident"], ok["lds"]) == (0, CU_LDS - PREC_STATIC_LDS, 1, 1, CU_LDS - PREC_STATIC_LDS)
    assert (over["slice"], budget["slice"]) == (CU_LDS - PREC_STATIC_LDS + 16, BUDGET)
    for got in (over, budget):
        assert (got["err"], got["msg"]) == (SF_ERR_UNSUPPORTED, "generic engine: one replica's LDS slice (with the precedence scratch / static copy) exceeds a CU's 160 KiB")
    assert plan(mixed(20905), prec_hbm=1)["msg"] == "model does not fit one wave's LDS slice"


# ---- invariants over a sweep ------------------------------------------------------------------------------------------------------------------
def _sweep_shape(rng):
    V = rng.choice((1, 2, 3, 5, 8, 10, 12, 20, 33, 64, 100))
    if rng.random() < 0.7:  # a precedence model, sometimes on a list class of a large element capacity
        n = int(2 ** rng.uniform(3, 13.6))
        capacity = n + (int(2 ** rng.uniform(8, 16.1)) if rng.random() < 0.35 else 0)
        if rng.random() < 0.25:  # a small graph (full copy, grouped trials) beside a list slice that leaves the groups little room
            n, capacity = rng.randint(20, 580), rng.randint(57000, 65535)
        pool = [LIST_CHANGE, LIST_SWAP, REVERSE, SUB_CHANGE, SUB_SWAP, KOPT, RUIN, PERMUTE, PRECEDENCE]
        kinds = rng.sample(pool, rng.randint(1, len(pool)))
        s = prec_shape(n, V, E=rng.randint(0, n - 1), owner=rng.random() < 0.5, capacity=min(capacity, 65535), kinds=kinds,
                       leg16=rng.randint(0, 1), levels=rng.choice((2, 3)))
        if rng.random() < 0.2:
            s.update(has_scalar=1, n_scalar=rng.choice((100, 1023, 1024, 4000)), n_values=rng.choice((20, 127, 128)), tables=rng.randint(0, 1))
    else:  # a list model with a distance meter: the default policy's leaves, or plain ones
        n = int(2 ** rng.uniform(4, 14.5))
        pool = [NEARBY_CHANGE, NEARBY_SWAP, SUB_CHANGE, SUB_SWAP, REVERSE, KOPT, RUIN] if rng.random() < 0.7 else [LIST_CHANGE, LIST_SWAP, REVERSE, KOPT, RUIN]
        kinds = rng.sample(pool, rng.randint(1, len(pool)))
        s = list_model(V, n, dim=n + 1, kopt_nearby=rng.randint(0, 1), leg16=rng.randint(0, 1), mat16=rng.randint(0, 1), small32=rng.randint(0, 1),
                       mat_symmetric=rng.randint(0, 1), levels=rng.choice((2, 4)), acceptor=rng.choice((1, 1, 3)), **leaves(*kinds))
        if rng.random() < 0.25:
            s.update(has_scalar=1, n_scalar=rng.choice((50, 1024, 3000)), n_values=rng.choice((8, 127, 300)), tables=rng.randint(0, 1), run_level=-1)
    s.update(n_replicas=rng.choice((1, 7, 256, 2048, 2049, 6144)), trace=int(rng.random() < 0.15))
    k = {}
    if rng.random() < 0.4:
        k = dict(prec_hbm=int(rng.random() < 0.2), prec_inc=int(rng.random() < 0.2), prec_no_sweep=int(rng.random() < 0.2), prec_static_hbm=int(rng.random() < 0.2),
                 prec_no_slim=int(rng.random() < 0.2), prec_no_occ=int(rng.random() < 0.2), no_fast=int(rng.random() < 0.2), wpb_max=rng.randint(1, 4))
        if rng.random() < 0.5:
            k.update(prec_groups_set=1, prec_groups=rng.choice((0, 2, 4, 8, 16)))
        if rng.random() < 0.3:
            k.update(prec_lds_max_set=1, prec_lds_max_kb=rng.choice((12, 36, 100)))
    return s, k


def test_invariants_of_accepted_plans(plan):
    """3,000 seeded shapes (precedence models, list models with a distance meter, either with a scalar class now and then) under random
    switches; the ranges refuse 172 of them (5.7 %), the bound is a quarter."""
    from solverforge_amd.director import decode_generic_launch_bits

    rng = random.Random(20260117)
    N, refused, seen = 3000, 0, {"groups": 0, "halved": 0, "mode2": 0, "fast": 0, "sweep": 0, "slim": 0, "hbm": 0}
    for _ in range(N):
        s, k = _sweep_shape(rng)
        got = plan(s, **k)
        if got["err"]:
            refused += 1
            assert got["msg"]
            continue
        static_lds = 0 if got["mode"] == 1 else (PREC_STATIC_LDS if got["prec"] else STATIC_LDS)
        assert got["wpb"] * got["slice"] + static_lds + got["prec_static"] <= CU_LDS, (s, k, got)
        assert got["resident"] >= 1 and 1 <= got["wpb"] <= k.get("wpb_max", 4) and got["resident"] % got["wpb"] == 0
        assert got["lds"] == got["wpb"] * got["slice"] + got["prec_static"] and got["block"] == 64 * got["wpb"]
        assert got["grid"] == -(-s["n_replicas"] // got["wpb"])
        assert got["prec"] == s.get("prec_on", 0) and (got["prec"] or not (got["prec_lds"] or got["prec_static"] or got["prec_groups"] or got["prec_sweep"]))
        if got["prec_groups"]:
            assert got["static"] == 1 and got["prec_lds"]
        if got["prec_static"]:
            assert got["prec_lds"]
        if got["prec_sweep"]:
            assert not got["prec_lds"] and not s["plf_on"] and not got["prec_inc"] and got["prec"]
        if got["mode"] == 2:
            assert got["prec_groups"] == 0 and got["prec"] and not s["trace"] and s["n_replicas"] > 2048
        if got["mode"] == 1:
            assert not got["prec"] and not s["trace"] and got["value_bytes"] == 2
        # A copy granted by the fit test against the estimate survives: without groups (forced off) the slice is the estimate -- or less,
        # with one-byte values -- and the chosen copy is the one that test left; the same copy stands in the final plan and passes the
        # same rule on the final slice, so the groups alone give way.
        if got["prec"]:
            est = plan(s, **dict(k, prec_groups_set=1, prec_groups=0))
            assert est["err"] == 0 and est["prec_groups"] == 0 and est["slice"] <= got["slice"]
            assert (got["prec_static"], got["prec_static_slim"], got["prec_lds"]) == (est["prec_static"], est["prec_static_slim"], est["prec_lds"]), (s, k)
            if got["prec_static"]:
                assert got["slice"] + 1024 + got["prec_static"] <= BUDGET, (s, k, got)
                unhalved = trials(s["prec_n"], s["V"], got["static"], k["prec_groups"] if k.get("prec_groups_set") else None)
                assert got["prec_groups"] <= unhalved
                seen["halved"] += got["prec_groups"] < unhalved
        want = {"fast": got["mode"] == 1, "node_global": bool(got["nodeg"]), "ring32": bool(got["ring32"]), "ruin": got["ruin_variant"],
                "value_bytes": got["value_bytes"], "prec": bool(got["prec"]), "prec_lds": bool(got["prec_lds"]), "prec_static": got["static"],
                "prec_groups": got["prec_groups"], "prec_occ": got["mode"] == 2, "prec_sweep": bool(got["prec_sweep"]),
                "prec_inc": bool(got["prec"] and got["prec_inc"]), "ruin_inst": bool(got["ruin_inst"]), "levels": got["levels"]}
        assert decode_generic_launch_bits(got["flags"]) == want, (s, k)
        for name, hit in (("groups", got["prec_groups"]), ("mode2", got["mode"] == 2), ("fast", got["mode"] == 1), ("sweep", got["prec_sweep"]),
                          ("slim", got["static"] == 2), ("hbm", got["prec"] and not got["prec_lds"])):
            seen[name] += bool(hit)
    assert refused < N // 4, refused
    assert all(v >= 10 for v in seen.values()), seen  # the sweep reaches every branch the properties speak of
