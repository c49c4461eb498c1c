// Launch plan of the generic N-leaf engine (k_mixed_search_wave: mixed models, the default list policy, every precedence model).
// Host only: sf_api.hip includes it after the engine sources (GCarve, the sizing functions, the SF_MIXED_* constants) and SF_LDS_BUDGET.
// launch_mixed describes the launch as a GenericShape, reads the diagnostic switches into GenericKnobs and asks plan_generic_launch, a pure
// function of the two, for everything the launch and sf_list_arith_flags need.  The structs hold int32 fields only: sf_debug_generic_plan
// hands them to the CPU tests (tests/test_generic_plan.py) as flat arrays in declaration order.
#pragma once

struct GenericShape {
    int32_t has_list, has_scalar;
    int32_t n_scalar, n_values, tables, run_level, run_P;  // scalar class (zeros without one): entities, values, ScalarModel::tables()
    int32_t V, n_cap, dim, leg16, small32, mat16, mat_symmetric, dist_level;  // list class (zeros without one)
    int32_t levels;                                        // score levels of the model
    int32_t n_leaves, kind[GL];                            // the union's leaves in launch order (sf_selector_kind)
    int32_t has_nearby, kopt_nearby, has_ruin;
    int32_t union_custom, union_order, acceptor, forager, order, dry_run, legacy_eval, explicit_seeds;
    int32_t prec_on, prec_n, prec_edges, prec_owner;       // ListPrecedenceMakespanConstraint: nodes, valid fixed edges, owners exist
    int32_t plf_on;                                        // critical-path leaf / route-graph filter / precedence-aware recreate tables in use
    int32_t n_replicas, trace;
};
// The SF_AMD_* diagnostic switches of the generic launch path (A/B runs and parity tests).
struct GenericKnobs {
    // read once per process: SF_AMD_MIXED_NO_FAST (force the general instantiation), SF_AMD_MIXED_NO_PRE_EVAL (score inside the replay),
    // SF_AMD_PREC_NO_OCC (never MODE 2), SF_AMD_DEBUG_LAUNCH (print the launch shape, once per change)
    int32_t no_fast, no_pre_eval, prec_no_occ, debug_launch;
    // read at every launch (tests toggle them inside one process)
    int32_t wpb_max;                            // SF_AMD_MIXED_WPB = 1..3: cap the replicas per workgroup (else 4)
    int32_t plf_slow, plf_force64;              // SF_AMD_PLF_SLOW, SF_AMD_PLF_FORCE64
    int32_t prec_hbm;                           // SF_AMD_PREC_HBM: force the HBM Kahn scratch
    int32_t prec_lds_max_set, prec_lds_max_kb;  // SF_AMD_PREC_LDS_MAX_KB: cap the LDS scratch (36 = the round-4 rule)
    int32_t prec_inc;                           // SF_AMD_PREC_INC: the incremental trial refresh (parity-complete but slower: profiles/r03f_precedence.txt)
    int32_t prec_static_hbm, prec_no_slim;      // SF_AMD_PREC_STATIC_HBM: leave the static graph in HBM / L1; SF_AMD_PREC_STATIC_SLIM=0: no slim copy
    int32_t prec_groups_set, prec_groups;       // SF_AMD_PREC_GROUPS = 0 / 2 / 4 / 8 / 16
    int32_t prec_no_sweep;                      // SF_AMD_PREC_NO_SWEEP: one full evaluation per trial with the HBM scratch too
};
static GenericKnobs generic_knobs() {
    auto on = [](const char* name) { return std::getenv(name) != nullptr ? 1 : 0; };
    static const GenericKnobs once{on("SF_AMD_MIXED_NO_FAST"), on("SF_AMD_MIXED_NO_PRE_EVAL"), on("SF_AMD_PREC_NO_OCC"), on("SF_AMD_DEBUG_LAUNCH")};
    GenericKnobs k = once;
    const char* e = std::getenv("SF_AMD_MIXED_WPB");
    k.wpb_max = e && std::atoi(e) >= 1 && std::atoi(e) < 4 ? std::atoi(e) : 4;
    k.plf_slow = on("SF_AMD_PLF_SLOW"), k.plf_force64 = on("SF_AMD_PLF_FORCE64"), k.prec_hbm = on("SF_AMD_PREC_HBM"), k.prec_inc = on("SF_AMD_PREC_INC");
    if ((e = std::getenv("SF_AMD_PREC_LDS_MAX_KB"))) k.prec_lds_max_set = 1, k.prec_lds_max_kb = std::atoi(e);
    k.prec_static_hbm = on("SF_AMD_PREC_STATIC_HBM"), k.prec_no_sweep = on("SF_AMD_PREC_NO_SWEEP");
    k.prec_no_slim = (e = std::getenv("SF_AMD_PREC_STATIC_SLIM")) && std::atoi(e) == 0 ? 1 : 0;
    if ((e = std::getenv("SF_AMD_PREC_GROUPS"))) k.prec_groups_set = 1, k.prec_groups = std::atoi(e);
    return k;
}

struct GenericPlan {
    int32_t err;                                   // SF_OK, or the refusal's code (`msg` says why; the launch shape and the flag word are not decided then)
    int32_t levels, value_bytes, ruin_inst, prec;  // the instantiation launch_tu_mixed<L, VTB, RUIN, PREC>
    int32_t mode;                                  // 0 general, 1 FAST, 2 the PREC build for four workgroups per CU
    int32_t nodeg, ring32;                         // node -> slot table in HBM; the 32-bit pre-evaluated delta ring
    int32_t ruin_variant;                          // 0 none / 1 general / 2 16-bit leg tables / 3 list-preserving (what the kernel's `v2` picks)
    int32_t prec_lds, prec_static, prec_static_slim, prec_groups, prec_sweep, prec_inc;  // as GLeaves carries them (prec_static in bytes)
    int32_t slice, wpb, grid, block, lds, resident;  // one replica's LDS bytes, replicas per workgroup, the launch, its dynamic LDS, resident replicas per CU
    int32_t flags;                                 // sf_generic_launch_bits
    const char* msg;
};

// One replica's LDS slice: the only place on the host that spells GCarve's argument list.  Its twin is the kernel's own carve in
// k_mixed_search_wave (sf_mixed_wave.hip, `const GCarve<VT> cv(...)`): the two must take the same arguments for the same launch.
// prec_words = the precedence constraint's node count when its Kahn scratch lives in the slice, else 0 (and then no groups either).
// The carve's ruin argument: 3 = the list-preserving recreate only (the FAST kernels), 2 = + 16-bit leg tables, 1 = the general path.
static size_t generic_slice_bytes(const GenericShape& s, int value_bytes, int prec_words, int prec_groups, bool nodeg) {
    // the scalar ruin-and-recreate leaf's block: the kernel reserves it in its TRACE instantiations when the union holds the leaf (kind 32768)
    const bool scalar_ruin = s.trace != 0 && has_scalar_ruin_leaf(s.kind, s.n_leaves);
    auto total = [&](auto vt) {
        return GCarve<decltype(vt)>(s.n_scalar, s.V, s.n_cap, s.has_nearby ? s.dim : 0, s.kopt_nearby, s.n_leaves, s.has_ruin ? (nodeg ? 3 : (s.leg16 ? 2 : 1)) : 0,
                                    s.dim, prec_words, s.tables ? s.n_values : 0, s.tables && s.run_level >= 0 ? s.run_P : 0, prec_groups, nodeg, scalar_ruin).total;
    };
    return value_bytes == 1 ? total(int8_t{}) : total(int16_t{});
}

// Pure: no context, no HIP call, no allocation, no environment.
static GenericPlan plan_generic_launch(const GenericShape& s, const GenericKnobs& k) {
    GenericPlan pl{};
    const bool PREC = s.prec_on != 0, RUIN = s.has_ruin != 0, trace = s.trace != 0;
    // two level counts (2, 4); i16 values, and i8 values for models whose scalar class dominates the LDS slice (a replica's value array
    // in one byte per entity: job shop 500 x 20 fits 4 waves per CU instead of 3).  The ruin leaf has i16 instantiations only.
    pl.levels = s.levels <= 2 ? 2 : 4;
    pl.value_bytes = !RUIN && s.has_scalar && s.n_values <= 127 && s.n_scalar >= 1024 ? 1 : 2;
    pl.ruin_inst = RUIN, pl.prec = PREC;
    // ---- precedence constraint: where the Kahn scratch, the static graph and the trial evaluation go ----
    // The whole-slice tests below run before the grouped trials are chosen, on an ESTIMATE of the slice: scratch in LDS, no grouped
    // evaluator, 2-byte values (the larger carve, also for a launch that takes one-byte values).
    const size_t est = PREC ? generic_slice_bytes(s, 2, s.prec_n, 0, false) : 0;
    // the Kahn scratch (12 bytes per node: prec_lds_scratch_bytes) goes to LDS while at least 4 replicas still fit a CU (up to 36 KiB =
    // 3,072 nodes) and beyond that whenever ONE replica per CU still fits: 10,000 nodes (job shop 500 x 20) run 1.7 x the rate of the HBM
    // scratch with half the replicas (profiles/r05_prec_eval_ab.txt)
    const size_t scratch = prec_lds_scratch_bytes(s.prec_n), lds_max = k.prec_lds_max_set ? (size_t)k.prec_lds_max_kb * 1024 : SF_LDS_BUDGET;
    bool fits = PREC && !k.prec_hbm && scratch <= lds_max && s.prec_n < 65535;
    if (fits && scratch > 36 * 1024) fits = est + 1024 <= SF_LDS_BUDGET;
    pl.prec_lds = fits ? 1 : 0, pl.prec_inc = k.prec_inc;
    // the constraint's static graph (durations, fixed successors / predecessors, in-degrees, owners) once per workgroup in LDS: every Kahn
    // round reads it behind a dependent LDS access
    if (PREC && pl.prec_lds && !k.prec_static_hbm) {
        const size_t b = prec_static_bytes(s.prec_n, s.prec_edges, s.prec_owner != 0);
        if (b <= 16 * 1024) pl.prec_static = (int32_t)b;
        // beyond that: the node records, fixed in-degrees and owners alone (what every evaluation reads per node; the rounds of a 1,000-node
        // evaluation waited on an L2 round trip for the record otherwise)
        const size_t sb = prec_static_slim_bytes(s.prec_n, s.prec_owner != 0);
        if (!pl.prec_static && sb <= 40 * 1024 && !k.prec_no_slim) pl.prec_static = (int32_t)sb, pl.prec_static_slim = 1;
        // the shared copy sits beside the replicas' slices in the workgroup's LDS: when one slice with the Kahn scratch in it leaves no room for
        // the copy (about 3,100 - 3,400 nodes without owners plus a large list slice), the copy stays in HBM instead of an over-size launch
        if (pl.prec_static && est + 1024 + (size_t)pl.prec_static > SF_LDS_BUDGET) pl.prec_static = 0, pl.prec_static_slim = 0;
    }
    // grouped trial evaluator (sf_prec_group.h): T trials per wavefront with private LDS scratch; its node records live in the FULL copy
    if (PREC && pl.prec_lds && pl.prec_static && !pl.prec_static_slim) {
        // default: as many trials per wave as the graph's width allows -- a Kahn round pops at most one node per list, so lane groups of
        // the largest power of two <= the list count (5 machines: 4 lanes, 16 trials; 10: 8 lanes, 8 trials) -- halved until the scratch
        // fits: under 14 KB, or the replica's precedence state (scratch + 16 B per node of Kahn arrays + ~2.5 KB) under 20 KB, which
        // keeps eight replicas on a CU.  200 nodes: 4; 300: 2; 1,000: off (50 x 20: 34.8 -> 26.0 M moves/s with 2)
        int T = 0, g = 1;
        while (g * 2 <= (s.V > 2 ? s.V : 2)) g *= 2;
        for (int t = 64 / g > 16 ? 16 : 64 / g; t >= 2; t >>= 1) {
            const size_t b = pgrp_bytes(s.prec_n, t, s.V);
            if (b <= 14 * 1024 || b + (size_t)s.prec_n * 16 + 2560 <= 20 * 1024) {
                T = t;
                break;
            }
        }
        if (k.prec_groups_set) {
            T = k.prec_groups;
            if (T != 2 && T != 4 && T != 8 && T != 16) T = 0;
            while (T > 1 && pgrp_bytes(s.prec_n, T, s.V) > 40 * 1024) T >>= 1;
        }
        pl.prec_groups = T > 1 ? T : 0;
    }
    // lane-per-trial sweep (prec_trial_sweep64): the default with the scratch in HBM
    pl.prec_sweep = PREC && !pl.prec_lds && !pl.prec_inc && !k.prec_no_sweep ? 1 : 0;
    if (s.plf_on) pl.prec_inc = pl.prec_sweep = 0;  // the critical-path leaf re-evaluates in the main scratch arrays: one full evaluation per trial
    // ---- FAST instantiation: the reference's default list policy on a list-only model (see k_mixed_search_wave) ----
    bool fast_kinds = true;  // the leaf kinds the FAST instantiation keeps (the default list policy of a slot with a distance meter)
    auto fast_kind = [&](int kd) { return kd == 16 || kd == 32 || kd == 64 || kd == 128 || kd == 256 || kd == 1024 || (kd == 512 && s.kopt_nearby); };
    for (int l = 0; l < s.n_leaves; ++l) fast_kinds = fast_kinds && fast_kind(s.kind[l]);
    const bool v2_ok = s.V <= 128 && s.n_cap <= 32767 && s.dim <= 32767 && s.small32 && s.mat16;  // rv2_model_ok (sf_ruin_v2.h)
    const bool fast = !k.no_fast && !trace && !PREC && pl.value_bytes == 2 && s.has_list && !s.has_scalar && s.acceptor == SF_ACCEPT_LATE_ACCEPTANCE &&
                      s.forager == SF_FORAGER_ACCEPTED_COUNT && !s.dry_run && !s.union_custom && s.union_order == SF_UNION_STRATIFIED_RANDOM && s.n_leaves > 1 &&
                      (s.mat_symmetric || s.dist_level < 0) && !s.legacy_eval && !s.explicit_seeds && fast_kinds &&
                      s.order == SF_ORDER_RANDOM &&  // (the default policy's SelectionOrder: compiled in, see StreamCtx in the kernel)
                      // with a ruin leaf the FAST kernel carries the list-preserving recreate only (sf_ruin_v2.h: rv2_model_ok + the edge table)
                      (!RUIN || (s.leg16 && v2_ok));
    // (FAST + ruin: the list-preserving recreate only and the node -> slot table in HBM, see the kernel)
    const bool nodeg = pl.nodeg = fast && (RUIN || SF_MIXED_FAST_NODEG != 0);
    pl.ring32 = fast && s.small32 && !k.no_pre_eval && !SF_MIXED_RING_LDS ? 1 : 0;  // the scoring stage stores 32-bit deltas
    pl.ruin_variant = !RUIN ? 0 : fast ? 3 : !s.leg16 ? 1 : v2_ok ? 3 : 2;
    // ---- the real slice ----
    auto slice = [&]() { return generic_slice_bytes(s, pl.value_bytes, pl.prec_lds ? s.prec_n : 0, pl.prec_lds ? pl.prec_groups : 0, nodeg); };
    size_t cv = slice();
    // The copy was sized against the estimate, which has no grouped scratch: when the real slice with the copy beside it fails the same fit
    // rule, the groups are halved until it passes.  Without them the slice is at most the estimate that passed, so the copy always stays.
    // (The rule's 1,024 bytes below SF_LDS_BUDGET matter: the PREC kernels hold SF_MIXED_PREC_STATIC_LDS bytes of static LDS, so a sum up
    // to the full 160 KiB is a launch the runtime rejects)
    while (pl.prec_groups && cv + 1024 + (size_t)pl.prec_static > SF_LDS_BUDGET) {
        pl.prec_groups = pl.prec_groups > 2 ? pl.prec_groups / 2 : 0;
        cv = slice();
    }
    pl.slice = (int32_t)cv;
    auto refuse = [&](const char* msg) { return pl.err = SF_ERR_UNSUPPORTED, pl.msg = msg, pl; };
    if (cv > SF_LDS_BUDGET) return refuse("model does not fit one wave's LDS slice");
    // precedence models: the four-workgroups-per-CU build when the launch has more replicas than two workgroups per CU hold and the LDS
    // slice lets more than eight share a CU (sf_mixed_wave.hip: MODE 2)
    // (not with the grouped evaluator: its scratch leaves room for 8 - 10 replicas per CU, and the 128-register build is slower per wave:
    // nine-leaf policy 20 x 10 at 6,144 replicas 71 M moves/s with it, 106 M without)
    const bool prec_occ = PREC && !trace && !k.prec_no_occ && !pl.prec_groups && s.n_replicas > 8 * 256 && (160 * 1024) / (cv + 256) > 8;
    pl.mode = fast ? 1 : (prec_occ ? 2 : 0);
    // replicas (waves) per workgroup: the count that keeps the most waves resident per CU (a workgroup's LDS is
    // allocated as a whole; the kernel is built for SF_MIXED_BLOCKS_PER_CU workgroups of 4 waves per CU, the FAST
    // instantiation for SF_MIXED_FAST_BLOCKS_PER_CU); ties go to the larger group
    const size_t max_waves = 4 * (size_t)(fast ? (RUIN ? SF_MIXED_FAST_RUIN_BLOCKS_PER_CU : SF_MIXED_FAST_BLOCKS_PER_CU) : (prec_occ ? SF_MIXED_PREC_BLOCKS_PER_CU : SF_MIXED_BLOCKS_PER_CU));  // by register budget
    size_t best_resident = 0;
    for (int w = 1; w <= k.wpb_max; ++w) {
        // + the kernel's static LDS (annealing state 1,024 bytes + the precedence paths' broadcast words; the FAST kernels have none), the shared copy of the precedence graph
        const size_t per_wg = cv * w + (fast ? 0 : (PREC ? SF_MIXED_PREC_STATIC_LDS : SF_MIXED_STATIC_LDS)) + (size_t)pl.prec_static;
        if (per_wg > 160 * 1024) break;
        size_t groups = (160 * 1024) / per_wg;
        if (groups * w > max_waves) groups = max_waves / w;
        if (groups * w >= best_resident) best_resident = groups * w, pl.wpb = w;
    }
    if (best_resident == 0) return refuse("generic engine: one replica's LDS slice (with the precedence scratch / static copy) exceeds a CU's 160 KiB");
    pl.resident = (int32_t)best_resident, pl.grid = (s.n_replicas + pl.wpb - 1) / pl.wpb, pl.block = 64 * pl.wpb, pl.lds = (int32_t)(cv * pl.wpb + (size_t)pl.prec_static);
    // recorded for sf_list_arith_flags: for a precedence model, where its scratch, static graph and trial evaluation went
    pl.flags = (fast ? SF_GEN_FAST : 0) | (nodeg ? SF_GEN_NODE_GLOBAL : 0) | (pl.ring32 ? SF_GEN_RING32 : 0) | (pl.ruin_variant << SF_GEN_RUIN_SHIFT) |
               (pl.value_bytes << SF_GEN_VT_SHIFT) | (RUIN ? SF_GEN_RUIN_INST : 0) | (pl.levels << SF_GEN_LEVELS_SHIFT);
    if (PREC)
        pl.flags |= SF_GEN_PREC | (pl.prec_lds ? SF_GEN_PREC_LDS : 0) | ((pl.prec_static ? (pl.prec_static_slim ? 2 : 1) : 0) << SF_GEN_PREC_STATIC_SHIFT) |
                    (pl.prec_groups << SF_GEN_PREC_GROUPS_SHIFT) | (prec_occ ? SF_GEN_PREC_OCC : 0) | (pl.prec_sweep ? SF_GEN_PREC_SWEEP : 0) |
                    (pl.prec_inc ? SF_GEN_PREC_INC : 0);
    return pl;
}
