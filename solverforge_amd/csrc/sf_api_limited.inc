// LimitedNeighborhood and the neighbourhoods of Variable Neighborhood Descent as compositions, on the host side (sf_mixed_wave.hip runs
// them, DESIGN 30 has the rules): sf_selector_limit, sf_union_limit, sf_vnd_set_neighborhoods, what a launch under them may run, and the
// LimitParams block of the launch.  Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

// selected_count_limit as the device holds it: a limit that a 32-bit pull count cannot reach is no limit
static uint32_t limit_word(int64_t v) { return v < 0 || v >= (int64_t)SF_LIMIT_NONE ? SF_LIMIT_NONE : (uint32_t)v; }

// MoveSelectorConfig::LimitedNeighborhood { selected_count_limit, selector: a leaf } (solverforge-config/src/move_selector.rs:34-109;
// SelectorComposition::Limited, composite.rs:72-89).  leaf_index = the zero-based order of the sf_selector_add* calls.
extern "C" int32_t sf_selector_limit(sf_ctx* ctx, int32_t leaf_index, int64_t selected_count_limit) {
    if (!ctx) return SF_ERR_INVALID;
    if (leaf_index < 0 || leaf_index >= (int32_t)ctx->selectors.size()) return fail(ctx, SF_ERR_INVALID, "sf_selector_limit: no such leaf");
    if (selected_count_limit < -1) return fail(ctx, SF_ERR_INVALID, "sf_selector_limit: selected_count_limit must be >= 0, or -1 for none");
    ctx->selectors[(size_t)leaf_index].limit = selected_count_limit;
    return SF_OK;
}

// LimitedNeighborhood { selector: the root union }
extern "C" int32_t sf_union_limit(sf_ctx* ctx, int64_t selected_count_limit) {
    if (!ctx) return SF_ERR_INVALID;
    if (selected_count_limit < -1) return fail(ctx, SF_ERR_INVALID, "sf_union_limit: selected_count_limit must be >= 0, or -1 for none");
    ctx->union_limit = selected_count_limit;
    return SF_OK;
}

// The neighbourhoods of Variable Neighborhood Descent as compositions (runtime/compiler/graph.rs:216-218 compiles them as it compiles the
// nodes of acceptor-forager search): contiguous groups of the declared leaves, a group of several leaves a union with equal weights under
// its own order, every group under its own limit.  Takes effect at the next sf_phase_start.
extern "C" int32_t sf_vnd_set_neighborhoods(sf_ctx* ctx, int32_t n_hoods, const int32_t* first_leaf, const int32_t* union_order, const int64_t* hood_limit) {
    if (!ctx) return SF_ERR_INVALID;
    if (n_hoods == 0) {  // one leaf each
        ctx->hoods_cfg = sf_ctx::HoodTable{};
        return SF_OK;
    }
    if (n_hoods < 0 || n_hoods > GL || !first_leaf || !union_order || !hood_limit) return fail(ctx, SF_ERR_INVALID, "sf_vnd_set_neighborhoods: bad arguments");
    if (first_leaf[0] != 0 || first_leaf[n_hoods] != (int32_t)ctx->selectors.size())
        return fail(ctx, SF_ERR_INVALID, "sf_vnd_set_neighborhoods: the neighbourhoods must cover the declared leaves");
    for (int32_t h = 0; h < n_hoods; ++h) {
        if (first_leaf[h + 1] <= first_leaf[h]) return fail(ctx, SF_ERR_INVALID, "sf_vnd_set_neighborhoods: a neighbourhood is empty or out of order");
        if (union_order[h] < SF_UNION_SEQUENTIAL || union_order[h] > SF_UNION_STRATIFIED_RANDOM) return fail(ctx, SF_ERR_INVALID, "sf_vnd_set_neighborhoods: union selection order");
        if (hood_limit[h] < -1) return fail(ctx, SF_ERR_INVALID, "sf_vnd_set_neighborhoods: a limit must be >= 0, or -1 for none");
    }
    sf_ctx::HoodTable t;
    t.first.assign(first_leaf, first_leaf + n_hoods + 1);
    t.order.assign(union_order, union_order + n_hoods);
    t.limit.assign(hood_limit, hood_limit + n_hoods);
    ctx->hoods_cfg = t;
    return SF_OK;
}

// Any limit or any grouping: such a context runs in the generic engine's TRACE instantiations whatever the model
static bool limited_any(const sf_ctx* ctx) {
    if (limit_word(ctx->union_limit) != SF_LIMIT_NONE || !ctx->hoods_cfg.first.empty()) return true;
    for (const auto& s : ctx->selectors)
        if (limit_word(s.limit) != SF_LIMIT_NONE) return true;
    return false;
}
// A limit that can bind: on a leaf, on the root union, or (under the phase that was started with them) on a neighbourhood
static bool limited_any_limit(const sf_ctx* ctx, bool vnd) {
    if (!vnd && limit_word(ctx->union_limit) != SF_LIMIT_NONE) return true;
    for (const auto& s : ctx->selectors)
        if (limit_word(s.limit) != SF_LIMIT_NONE) return true;
    if (vnd)
        for (int64_t v : ctx->hoods.limit)
            if (limit_word(v) != SF_LIMIT_NONE) return true;
    return false;
}

// What a launch under a limit or a grouping cannot run (DESIGN 30).  nullptr, or the reason of the refusal.
static const char* limited_launch_refusal(const sf_ctx* ctx, bool vnd) {
    if (ctx->engine != SF_ENGINE_AUTO)
        return "limited neighbourhood / neighbourhood groups: the generic engine only (a block, wave or scalar engine was forced: sf_solver_set_engine)";
    if (!limited_any_limit(ctx, vnd)) return nullptr;
    for (const auto& s : ctx->selectors) {
        if (s.kind == SF_SEL_LIST_RUIN) return "limited neighbourhood: not around a union that holds the list ruin leaf (how a cut cursor leaves its per-solve stream is not restated)";
        if (s.kind == SF_SEL_SCALAR_RUIN) return "limited neighbourhood: not around a union that holds the scalar ruin leaf (how a cut cursor leaves its per-solve stream is not restated)";
        if (s.kind == SF_SEL_LIST_PRECEDENCE) return "limited neighbourhood: not around a union that holds the critical-path leaf (its trials are scored at cursor open)";
    }
    return nullptr;
}

// The LimitParams of a launch whose leaves `gl` lists (launch_mixed has filled gl.lim.leaf beside gl.kind).  0, or the error code.
static int limited_fill(sf_ctx* ctx, GLeaves& gl, bool vnd, bool trace) {
    gl.lim.root = vnd ? SF_LIMIT_NONE : limit_word(ctx->union_limit);
    gl.lim.n_hoods = 0;
    for (int h = 0; h < GL; ++h) gl.lim.hood_limit[h] = SF_LIMIT_NONE;
    if (vnd && !ctx->hoods.first.empty()) {
        const int n = (int)ctx->hoods.order.size();
        if (ctx->hoods.first[(size_t)n] != gl.n) return fail(ctx, SF_ERR_INVALID, "variable neighborhood descent: the neighbourhood table does not cover the leaves of the launch");
        gl.lim.n_hoods = n;
        for (int h = 0; h <= n; ++h) gl.lim.hood_first[h] = (uint8_t)ctx->hoods.first[(size_t)h];
        for (int h = 0; h < n; ++h) gl.lim.hood_order[h] = (uint8_t)ctx->hoods.order[(size_t)h], gl.lim.hood_limit[h] = limit_word(ctx->hoods.limit[(size_t)h]);
    }
    bool any = gl.lim.root != SF_LIMIT_NONE || gl.lim.n_hoods > 0;
    for (int l = 0; l < gl.n; ++l) any = any || gl.lim.leaf[l] != SF_LIMIT_NONE;
    if (any && !trace) return fail(ctx, SF_ERR_INVALID, "limited neighbourhood: the traced instantiation carries it");
    return SF_OK;
}
