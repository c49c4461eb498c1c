// Scalar ruin-and-recreate leaf on the host side (csrc/sf_scalar_ruin.h holds the rules, sf_mixed_wave.hip runs them): the selector, the
// per-solve streams at phase start, what a launch with the leaf may run, and the batch table of a traced / generated step.
// Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

// RuinRecreateMoveSelectorConfig (solverforge-config/src/move_selector.rs:299-328) -> ScalarRuinRecreateSpec (scalar_neighborhood/spec.rs:122-139)
extern "C" int32_t sf_selector_add_scalar_ruin(sf_ctx* ctx, int32_t d, int32_t var, int32_t min_ruin_count, int32_t max_ruin_count, int32_t moves_per_step,
                                               int32_t value_candidate_limit, int32_t recreate_heuristic, const char* variable_name) {
    if (!ctx) return SF_ERR_INVALID;
    if (ctx->initialized) return fail(ctx, SF_ERR_INVALID, "selectors are frozen after sf_initialize");
    if (min_ruin_count < 1) return fail(ctx, SF_ERR_INVALID, "scalar ruin: min_ruin_count must be at least 1");  // spec.rs:126-131
    if (max_ruin_count < min_ruin_count) return fail(ctx, SF_ERR_INVALID, "scalar ruin: max_ruin_count must be >= min_ruin_count");
    if (moves_per_step < 0 || value_candidate_limit < -1) return fail(ctx, SF_ERR_INVALID, "scalar ruin: negative moves_per_step / value_candidate_limit below -1");
    if (recreate_heuristic != SF_RECREATE_FIRST_FIT && recreate_heuristic != SF_RECREATE_CHEAPEST_INSERTION)
        return fail(ctx, SF_ERR_INVALID, "scalar ruin: recreate heuristic must be first fit or cheapest insertion");
    if (max_ruin_count > (int32_t)SRUIN_MAX_COUNT) return fail(ctx, SF_ERR_UNSUPPORTED, "scalar ruin: at most 8 entities per move on the device");
    if (moves_per_step > (int32_t)SRUIN_MAX_MOVES) return fail(ctx, SF_ERR_UNSUPPORTED, "scalar ruin: at most 16 moves per step on the device");
    for (auto& s : ctx->selectors)
        if (s.kind == SF_SEL_SCALAR_RUIN && s.desc == d && s.var == var) return fail(ctx, SF_ERR_UNSUPPORTED, "one scalar ruin leaf per scalar variable");
    SelectorSpec s{SF_SEL_SCALAR_RUIN, d, var, 0, -1};
    s.min_size = min_ruin_count;
    s.max_size = max_ruin_count;
    s.moves_per_step = moves_per_step == 0 ? 10 : moves_per_step;  // moves_per_step.unwrap_or(10).max(1)
    s.value_limit = value_candidate_limit;
    s.recreate = recreate_heuristic;
    s.variable_name = variable_name ? variable_name : "";
    ctx->selectors.push_back(s);
    return SF_OK;
}

// sf_step_evaluate, sf_apply and sf_step_decide* given an SF_MOVE_SCALAR_RUIN record (sf_api_moves.inc)
static const char* const SCALAR_RUIN_RECORD_REFUSAL =
    "an SF_MOVE_SCALAR_RUIN record names a row of its step's batch table, not a move: pass the edits of sf_get_scalar_ruin_table through the compound calls";

static const SelectorSpec* scalar_ruin_selector(const sf_ctx* ctx) {
    for (auto& s : ctx->selectors)
        if (s.kind == SF_SEL_SCALAR_RUIN && ctx->has_scalar_model && s.desc == ctx->scalar_desc) return &s;
    return nullptr;
}

// scalar_neighborhood/cursor.rs:234-256: replica r's stream = SmallRng::seed_from_u64(scoped_seed(random_seed + r, descriptor, variable,
// "scalar_ruin_recreate_move_selector")); every cursor open of the solve draws from it
static int scalar_ruin_phase_start(sf_ctx* ctx) {
    const SelectorSpec* rs = scalar_ruin_selector(ctx);
    if (!rs) return SF_OK;
    if (!ctx->d_sruin_rng) {
        int rc = dalloc(ctx, &ctx->d_sruin_rng, (size_t)ctx->R * 4);
        if (!rc) rc = dalloc(ctx, &ctx->d_sruin_table, (size_t)SRUIN_TAB_WORDS);
        if (rc) return rc;
    }
    std::vector<uint64_t> st((size_t)ctx->R * 4);
    for (int r = 0; r < ctx->R; ++r) {
        uint64_t state = scoped_seed(ctx->cfg.random_seed + (uint64_t)r, (uint64_t)rs->desc, rs->variable_name, "scalar_ruin_recreate_move_selector");
        for (int i = 0; i < 4; ++i) {  // xoshiro256++ seed_from_u64: splitmix64 expansion
            state += 0x9E3779B97F4A7C15ULL;
            uint64_t z = state;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            st[(size_t)r * 4 + i] = z ^ (z >> 31);
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_sruin_rng, st.data(), st.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_sruin_table, 0, (size_t)SRUIN_TAB_WORDS * 4, ctx->stream));  // no step of this phase yet
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

// What a launch whose union holds the leaf cannot run (DESIGN 29).  nullptr, or the reason of the refusal.  (TabuSearch and Variable
// Neighborhood Descent name the leaf in their own refusals.)
static const char* scalar_ruin_launch_refusal(sf_ctx* ctx) {
    if (ctx->engine != SF_ENGINE_AUTO) return "scalar ruin leaf: the generic engine only (a block or wave engine was forced: sf_solver_set_engine)";
    if (ctx->xown_level >= 0) return "scalar ruin leaf: the join of the two planning classes is not priced by the leaf's recreate";
    if (ctx->nearby_scalar_dynamic) return "scalar ruin leaf: not beside a dynamic nearby scalar slot";
    return nullptr;
}

extern "C" int32_t sf_get_scalar_ruin_table(sf_ctx* ctx, int32_t replica, int32_t* out_counts, int32_t* out_entities, int32_t* out_values, int32_t* out_emitted) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized || replica < 0 || replica >= ctx->R || !out_counts || !out_entities || !out_values || !out_emitted)
        return fail(ctx, SF_ERR_INVALID, "bad sf_get_scalar_ruin_table");
    if (!scalar_ruin_selector(ctx) || !ctx->d_sruin_table) return fail(ctx, SF_ERR_INVALID, "sf_get_scalar_ruin_table: no scalar ruin leaf, or no phase was started with it");
    int32_t tab[SRUIN_TAB_WORDS];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(tab, ctx->d_sruin_table, sizeof(tab), hipMemcpyDeviceToHost));
    if (tab[SRUIN_TAB_REPLICA + 1] == 0 || tab[SRUIN_TAB_REPLICA] != replica)
        return fail(ctx, SF_ERR_INVALID, "sf_get_scalar_ruin_table: the replica's last step was neither traced nor generated");
    std::memcpy(out_counts, tab + SRUIN_TAB_CNT, SRUIN_MAX_MOVES * 4);
    std::memcpy(out_entities, tab + SRUIN_TAB_ENT, SRUIN_MAX_MOVES * SRUIN_MAX_COUNT * 4);
    std::memcpy(out_values, tab + SRUIN_TAB_VAL, SRUIN_MAX_MOVES * SRUIN_MAX_COUNT * 4);
    std::memcpy(out_emitted, tab + SRUIN_TAB_EMIT, SRUIN_MAX_MOVES * 4);
    return SF_OK;
}
