// Variable Neighborhood Descent on the host side (csrc/sf_step.h holds the rules, sf_mixed_wave.hip runs them): the local-search type
// (sf_solver_configure_vnd), the state rows at phase start, what a launch under it may run, sf_get_vnd_state and sf_vnd_done_count.
// Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

// LocalSearchType::VariableNeighborhoodDescent (solverforge-config/src/phase.rs:148-155): the neighbourhoods are the context's declared
// leaves in declaration order, one leaf each (or the groups of sf_vnd_set_neighborhoods, sf_api_limited.inc), compiled with
// SelectionOrder::Original (runtime/compiler/local_search.rs:55-89).  The
// acceptor, forager, random-ties, selection-order and union settings are ignored while it holds; sf_solver_configure (and
// sf_solver_configure_default, which calls it) returns the context to acceptor-forager search.
extern "C" int32_t sf_solver_configure_vnd(sf_ctx* ctx) {
    if (!ctx) return SF_ERR_INVALID;
    ctx->vnd = true;
    return SF_OK;
}

// The neighbourhoods of the context: the declared leaves of its planning classes, as launch_mixed lists them
static int vnd_neighbourhoods(const sf_ctx* ctx) {
    int n = 0;
    for (const auto& s : ctx->selectors) {
        const bool is_list = s.kind != SF_SEL_SCALAR_CHANGE && s.kind != SF_SEL_SCALAR_SWAP && s.kind != SF_SEL_NEARBY_SCALAR_CHANGE && s.kind != SF_SEL_NEARBY_SCALAR_SWAP &&
                             s.kind != SF_SEL_SCALAR_RUIN;
        if (is_list ? (ctx->has_list_model && s.desc == ctx->list_desc) : (ctx->has_scalar_model && s.desc == ctx->scalar_desc)) n += 1;
    }
    return n;
}

// sf_phase_start under the phase: zeros and n in every replica's row; the phase-start kernels set k and the done flag (vnd_phase_started).
// `st` = the R rows about to be uploaded.
static void vnd_phase_rows(sf_ctx* ctx, std::vector<uint64_t>& st) {
    // the neighbourhoods of the phase: one declared leaf each, or the groups sf_vnd_set_neighborhoods set (sf_api_limited.inc) -- k and n
    // count neighbourhoods either way
    ctx->hoods = ctx->hoods_cfg;
    ctx->vnd_leaves = vnd_neighbourhoods(ctx);
    ctx->vnd_n = ctx->hoods.first.empty() ? ctx->vnd_leaves : (int)ctx->hoods.order.size();
    for (int r = 0; r < ctx->R; ++r) {
        uint64_t* w = st.data() + (size_t)r * SA_WORDS;
        std::fill(w, w + SA_WORDS, (uint64_t)0);
        w[VND_N] = (uint64_t)ctx->vnd_n;
    }
}

// What a launch under the phase cannot run (DESIGN 27).  nullptr, or the reason of the refusal.  (More leaves than a union holds are
// refused by launch_mixed, as for every union.)
static const char* vnd_launch_refusal(sf_ctx* ctx) {
    if (ctx->engine != SF_ENGINE_AUTO)
        return "variable neighborhood descent: the generic engine only (a block or wave engine was forced: sf_solver_set_engine)";
    for (const auto& s : ctx->selectors) {
        if (s.kind == SF_SEL_LIST_RUIN)
            return "variable neighborhood descent: the ruin leaf (its per-solve random stream and step-start trials have no Original-order meaning)";
        if (s.kind == SF_SEL_SCALAR_RUIN)
            return "variable neighborhood descent: the scalar ruin leaf (its per-solve random stream and step-start trials have no Original-order meaning)";
        if (s.kind == SF_SEL_LIST_PRECEDENCE)
            return "variable neighborhood descent: the critical-path precedence leaf (its gated multi-swaps and step analysis are not a plain neighbourhood)";
    }
    return nullptr;
}

extern "C" int32_t sf_get_vnd_state(sf_ctx* ctx, int32_t replica, int32_t* out_k, int32_t* out_n, int32_t* out_done, uint64_t* out_idle_steps) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->search_alloc || replica < 0 || replica >= ctx->R || !out_k || !out_n || !out_done || !out_idle_steps)
        return fail(ctx, SF_ERR_INVALID, "bad sf_get_vnd_state");
    if (ctx->sp.acceptor != VND_KIND) return fail(ctx, SF_ERR_INVALID, "sf_get_vnd_state: the phase was not started under variable neighborhood descent");
    uint64_t w[VND_WORDS];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(w, ctx->sp.sa.state + (size_t)replica * SA_WORDS, sizeof(w), hipMemcpyDeviceToHost));
    *out_k = (int32_t)w[VND_K], *out_n = (int32_t)w[VND_N], *out_done = (int32_t)w[VND_DONE], *out_idle_steps = w[VND_IDLE];
    return SF_OK;
}

// The replicas at k == n: one strided read of the done words, 8 bytes per replica
extern "C" int32_t sf_vnd_done_count(sf_ctx* ctx, int32_t* out) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->search_alloc || !out) return fail(ctx, SF_ERR_INVALID, "bad sf_vnd_done_count");
    if (ctx->sp.acceptor != VND_KIND) return fail(ctx, SF_ERR_INVALID, "sf_vnd_done_count: the phase was not started under variable neighborhood descent");
    std::vector<uint64_t> done((size_t)ctx->R);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy2D(done.data(), 8, ctx->sp.sa.state + VND_DONE, (size_t)SA_WORDS * 8, 8, (size_t)ctx->R, hipMemcpyDeviceToHost));
    int32_t n = 0;
    for (uint64_t d : done) n += d != 0 ? 1 : 0;
    *out = n;
    return SF_OK;
}
