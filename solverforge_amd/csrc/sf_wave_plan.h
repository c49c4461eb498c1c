// Launch plan of the wave engine (k_list_search_wave: list models under the two nearby leaves of the default policy).
// Host only: sf_api.hip includes it after the engine sources (WCarve, node_slot_compact_ok, WPB, SF_WAVES_PER_EU) and SF_LDS_BUDGET.
// launch_list_wave describes the launch as a WaveShape, reads the diagnostic switches into WaveKnobs and asks plan_wave_launch, a pure
// function of the two, for everything the launch and sf_list_wave_layout need; engine resolution asks wave_engine_fits / wave_engine_default
// of the same shape.  The structs hold int32 fields only: sf_debug_wave_plan hands them to the CPU tests (tests/test_wave_plan.py) as flat
// arrays in declaration order.
#pragma once

struct WaveShape {
    // the presorted neighbour index exists (a matrix meter, <= 16384 nodes); the list class; the largest max_nearby of its nearby selectors (1 without one)
    int32_t nbr_index, V, n_cap, dim, max_nearby;
    int32_t levels, mat32, mat16, small, dist_level;  // score levels of the model; ListModel::mat32 / mat16 exist; sf_ctx::lm_small
    int32_t acceptor, forager, order, dry_run;
    int32_t n_leaves, kind[MAX_LEAVES];  // the launch's leaves in order (sf_selector_kind)
    int32_t n_replicas, trace;
};
// The SF_AMD_* diagnostic switches of the wave launch path (A/B runs and parity tests).
struct WaveKnobs {
    // read once per process: SF_AMD_NO_COMPACT (never a COMPACT slice), SF_AMD_WAVE_WPE (cap the waves per SIMD: 4 / 5 / 6)
    int32_t no_compact, max_wpe;
    // read at every launch (tests toggle them inside one process)
    int32_t wpb_max;      // SF_AMD_WAVE_WPB = 1..3: cap the replicas per workgroup (else WPB)
    int32_t node_global;  // SF_AMD_NODE_GLOBAL: 0 = never, 1 = whenever a COMPACT slice is taken, else (-1 unset) the rule
};
static WaveKnobs wave_knobs() {
    static const WaveKnobs once{std::getenv("SF_AMD_NO_COMPACT") != nullptr ? 1 : 0, std::getenv("SF_AMD_WAVE_WPE") ? std::atoi(std::getenv("SF_AMD_WAVE_WPE")) : 6};
    WaveKnobs k = once;
    const char* e = std::getenv("SF_AMD_WAVE_WPB");
    k.wpb_max = e && std::atoi(e) >= 1 && std::atoi(e) < WPB ? std::atoi(e) : WPB;
    k.node_global = (e = std::getenv("SF_AMD_NODE_GLOBAL")) ? std::atoi(e) : -1;
    return k;
}

struct WavePlan {
    int32_t err;                  // SF_OK, or the refusal's code (`msg` says why; nothing else is decided then)
    int32_t levels;               // the instantiation launch_tu_list_wave<L>
    int32_t mode;                 // 0 general, 1 FAST, 2 FAST + SMALL, 3 / 4 / 5 + COMPACT built for 4 / 5 / 6 waves per SIMD, 6 + NODEG (sf_list_wave_layout)
    int32_t compact, wpe, nodeg;  // what the mode means: COMPACT slice, waves per SIMD of the build, node -> slot table in HBM
    int32_t slice, wpb, grid, block, lds, resident;  // one replica's LDS bytes, replicas per workgroup, the launch, its dynamic LDS, resident replicas per CU
    const char* msg;
};

// One replica's LDS slice: the only place on the host that spells WCarve's argument list.  Its twin is the kernel's own carve in
// k_list_search_wave (sf_list_wave.hip, `const WCarve cv(...)`): the two must take the same arguments for the same launch.
static size_t wave_slice_bytes(const WaveShape& s, bool compact, bool node_global) {
    return WCarve(s.V, s.n_cap, s.dim, s.max_nearby, compact, node_global).total;
}
// Engine resolution.  The engine can run the model: the neighbour index, u16 element ids / ordinals in LDS, and one replica's (wide) slice
// fits a CU.  It is the default when the slice leaves room for several replicas per CU: at most half the budget.
static bool wave_engine_fits(const WaveShape& s, size_t budget = SF_LDS_BUDGET) {
    return s.nbr_index && s.dim <= 16384 && s.n_cap + s.V <= 65535 && s.max_nearby <= 64 && wave_slice_bytes(s, false, false) <= budget;
}
static bool wave_engine_default(const WaveShape& s) { return wave_engine_fits(s, SF_LDS_BUDGET / 2); }

// Replicas (waves) per workgroup for a slice: the count <= wpb_max that keeps the most replicas resident per CU (a workgroup's LDS is
// allocated whole: whole workgroups in 160 KiB), at most wave_cap of them by the build's register budget; ties go to the larger group.
struct WaveFit { int32_t slice, resident, wpb; };
static WaveFit wave_fit(size_t slice, size_t wave_cap, bool fast, int wpb_max) {
    WaveFit f{(int32_t)slice, 0, 1};
    for (size_t w = 1; w <= (size_t)wpb_max && slice * w <= SF_LDS_BUDGET; ++w) {
        size_t groups = (160 * 1024) / (slice * w + (fast ? 0 : 1024));  // + the static annealing state (the FAST instantiations have none)
        if (groups * w > wave_cap) groups = wave_cap / w;
        if (groups * w >= (size_t)f.resident) f.resident = (int32_t)(groups * w), f.wpb = (int32_t)w;
    }
    return f;
}

// Pure: no context, no HIP call, no allocation, no environment.
static WavePlan plan_wave_launch(const WaveShape& s, const WaveKnobs& k) {
    WavePlan pl{};
    if (!wave_engine_fits(s))
        return pl.err = SF_ERR_UNSUPPORTED, pl.msg = "wave engine cannot run this model (needs a nearby matrix meter, <= 65535 elements, LDS slice <= 160 KiB)", pl;
    // kernels are instantiated for 2 and 4 score levels; 1- and 3-level models run with one padded
    // (always zero) least-significant level, which never changes a lexicographic comparison
    pl.levels = s.levels <= 2 ? 2 : 4;
    const bool fast = !s.trace && s.mat32 && s.dist_level >= 0 && s.acceptor == 1 && s.forager == 0 && !s.dry_run && s.n_leaves == 2 &&
                      s.kind[0] == SF_SEL_NEARBY_LIST_CHANGE && s.kind[1] == SF_SEL_NEARBY_LIST_SWAP && s.order == SF_ORDER_RANDOM;
    pl.mode = fast ? (s.small ? 2 : 1) : 0;
    const size_t cap4 = 4 * SF_WAVES_PER_EU;
    const WaveFit wide = wave_fit(wave_slice_bytes(s, false, false), cap4, fast, k.wpb_max);
    WaveFit pick = wide;
    if (pl.mode == 2 && node_slot_compact_ok(s.V) && s.mat16 && !k.no_compact) {  // (the COMPACT kernels gather from the u16 matrix)
        // the COMPACT slice when it puts more replicas on a CU: CVRP-5000 5 instead of 3 (LDS-bound, compiled for 4 waves per SIMD);
        // CVRP-1000 20 / 24 instead of 16 with the instantiations compiled for 5 / 6 waves per SIMD (6: 80 VGPRs)
        const size_t slice = wave_slice_bytes(s, true, false);
        const WaveFit c4 = wave_fit(slice, cap4, fast, k.wpb_max), c5 = wave_fit(slice, 20, fast, k.wpb_max), c6 = wave_fit(slice, 24, fast, k.wpb_max);
        // large models: the node -> slot table in HBM when that puts more replicas on a CU (a wave runs as fast at CVRP-5000 as at
        // CVRP-1000; the slice decides how many are resident: 29 KB = 5 per CU, 14 KB = 11)
        const WaveFit g = wave_fit(wave_slice_bytes(s, true, true), cap4, fast, k.wpb_max);
        if (k.max_wpe >= 6 && c6.resident > 20 && c6.resident > wide.resident) pl.mode = 5, pick = c6;
        else if (k.max_wpe >= 5 && c5.resident > 16 && c5.resident > wide.resident) pl.mode = 4, pick = c5;
        else if (c4.resident > wide.resident) pl.mode = 3, pick = c4;
        // (only after a COMPACT mode was taken, and by the rule from mode 3 alone: DESIGN, "Wave launch plan")
        if (pl.mode >= 3 && k.node_global != 0 && (k.node_global == 1 || (pl.mode == 3 && g.resident > c4.resident))) pl.mode = 6, pick = g;
    }
    pl.compact = pl.mode >= 3, pl.nodeg = pl.mode == 6, pl.wpe = pl.mode == 5 ? 6 : pl.mode == 4 ? 5 : SF_WAVES_PER_EU;
    pl.slice = pick.slice, pl.wpb = pick.wpb, pl.resident = pick.resident;
    pl.grid = (s.n_replicas + pl.wpb - 1) / pl.wpb, pl.block = 64 * pl.wpb, pl.lds = pl.slice * pl.wpb;
    return pl;
}
