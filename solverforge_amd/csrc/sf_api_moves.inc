// Host-driven step surface of the C ABI: one call scores a batch of the host's moves (sf_step_evaluate, sf_step_evaluate_compound),
// decides a step over a candidate provider's output (sf_step_decide*) or commits one move (sf_apply, sf_apply_compound).  Every
// device buffer of a call is a Scratch (sf_api.hip): it is freed on every return, and hipFree is the fence of a return that
// leaves kernels queued.  Included into sf_api.hip (same translation unit).

extern "C" {

// SF_MOVE_LIST_RUIN entries of a host batch: one wavefront each (csrc/sf_construct.hip)
static int launch_ruin_moves(sf_ctx* ctx, int replica, const int32_t* d_moves, const std::vector<int32_t>& which, int64_t* d_sc, int32_t* d_do, int commit) {
    const RuinMoveCarve cv(ctx->lm.V, ctx->lm.n_cap);
    if (ctx->lm.n_cap > 65535 || ctx->lm.dim > 65536 || cv.total > SF_LDS_BUDGET)
        return fail(ctx, SF_ERR_UNSUPPORTED, "list ruin moves: the list class must fit one wave's LDS slice with 16-bit elements");
    const SelectorSpec* rs = ruin_selector(ctx);
    const int skip_empty = rs ? rs->skip_empty : 0;
    Scratch<int32_t> d_idx;
    if (int rc = d_idx.upload(ctx, which.data(), which.size())) return rc;
    const auto kern = ctx->levels <= 2 ? k_list_ruin_moves<2> : k_list_ruin_moves<4>;
    hipError_t e = launch_with_lds(kern, dim3((unsigned)which.size()), dim3(64), cv.total, ctx->stream, ctx->lm, replica, d_moves, d_idx.p, d_sc, d_do, skip_empty, commit);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_rc(ctx, e);
}

// SF_MOVE_LIST_RUIN records on a precedence model: k_prec_ruin_moves, at most R records per launch (one scratch slot each)
static int launch_prec_ruin_moves(sf_ctx* ctx, int replica, const int32_t* d_moves, const std::vector<int32_t>& which, int64_t* d_sc, int32_t* d_do, int commit) {
    if (ctx->lm.dist_level >= 0 || ctx->lm.cap_level >= 0)
        return fail(ctx, SF_ERR_UNSUPPORTED, "list ruin move on a precedence model with distance / capacity constraints");
    if (int rc = ensure_plf(ctx)) return rc;
    const size_t lds = (((size_t)ctx->lm.V + 1 + 3) & ~(size_t)3) * 4 + (size_t)ctx->lm.n_cap * 2 + 16;
    if (ctx->lm.n_cap > 65535 || lds > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "list ruin moves: the list class must fit one wave's LDS slice with 16-bit elements");
    const SelectorSpec* rs = ruin_selector(ctx);
    const int skip_empty = rs ? rs->skip_empty : 0;
    Scratch<int32_t> d_idx;
    if (int rc = d_idx.upload(ctx, which.data(), which.size())) return rc;
    hipError_t e = hipFuncSetAttribute((const void*)k_prec_ruin_moves, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    for (size_t base = 0; base < which.size() && e == hipSuccess; base += (size_t)ctx->R) {
        const unsigned chunk = (unsigned)std::min<size_t>((size_t)ctx->R, which.size() - base);
        hipLaunchKernelGGL(k_prec_ruin_moves, dim3(chunk), dim3(64), lds, ctx->stream, ctx->lm, ctx->pm, ctx->plf, replica, d_moves, d_idx.p + base, d_sc, d_do, commit,
                           prec_level_order(ctx), ctx->prec_policy ? 1 : 0, skip_empty);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_rc(ctx, e);
}

int32_t sf_step_evaluate(sf_ctx* ctx, int32_t replica, const sf_move_t* moves, int64_t n, int64_t* out_scores,
                         int32_t* out_doable) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (replica < 0 || replica >= ctx->R || n < 0 || !moves || !out_scores || !out_doable)
        return fail(ctx, SF_ERR_INVALID, "bad sf_step_evaluate arguments");
    if (ctx->xown_level >= 0)
        for (int64_t i = 0; i < n; ++i)
            if (moves[i].kind == SF_MOVE_LIST_RUIN) return fail(ctx, SF_ERR_UNSUPPORTED, "the join of the two planning classes is not priced by a ruin's recreate");
    for (int64_t i = 0; i < n; ++i)
        if (moves[i].kind == SF_MOVE_SCALAR_RUIN) return fail(ctx, SF_ERR_UNSUPPORTED, SCALAR_RUIN_RECORD_REFUSAL);
    if (n == 0) return SF_OK;
    Scratch<sf_move_t> d_rec;
    Scratch<int64_t> d_sc;
    Scratch<int32_t> d_do;
    int rc;
    if ((rc = d_rec.upload(ctx, moves, (size_t)n)) || (rc = d_sc.alloc(ctx, (size_t)n * ctx->levels)) || (rc = d_do.alloc(ctx, (size_t)n))) return rc;
    const int32_t* d_moves = (const int32_t*)d_rec.p;
    int grid = (int)((n + 255) / 256);
    const int mixed = ctx->has_list_model && ctx->has_scalar_model;
    if (mixed) {
        (void)hipMemsetAsync(d_sc.p, 0, (size_t)n * ctx->levels * 8, ctx->stream);
        (void)hipMemsetAsync(d_do.p, 0, (size_t)n * 4, ctx->stream);
    }
    if (ctx->has_list_model)
        hipLaunchKernelGGL(k_list_evaluate_moves, dim3(grid), dim3(256), 0, ctx->stream, ctx->lm, replica, d_moves, n, d_sc.p, d_do.p, mixed);
    if (ctx->has_scalar_model)
        HIPCHK(ctx, launch_with_lds(k_scalar_evaluate_moves, dim3(grid), dim3(256), scalar_table_bytes(ctx), ctx->stream, ctx->sm, replica, d_moves, n, d_sc.p, d_do.p, mixed));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && ctx->has_list_model) {  // list ruin moves: scored by their own kernel, one wavefront per move
        std::vector<int32_t> which;
        for (int64_t i = 0; i < n; ++i)
            if (moves[i].kind == SF_MOVE_LIST_RUIN) which.push_back((int32_t)i);
        // precedence model: the recreate is scored by the precedence constraint (k_prec_ruin_moves)
        if (!which.empty() && (rc = ctx->pm.on ? launch_prec_ruin_moves(ctx, replica, d_moves, which, d_sc.p, d_do.p, 0)
                                               : launch_ruin_moves(ctx, replica, d_moves, which, d_sc.p, d_do.p, 0)))
            return rc;
    }
    if (e == hipSuccess && ctx->has_list_model && ctx->pm.on) {  // precedence delta of every doable list move: one wavefront per record
        const PrecMoveCarve cv(ctx->lm.V, ctx->lm.n_cap);
        if (ctx->lm.n_cap > 65535 || cv.total > SF_LDS_BUDGET)
            return fail(ctx, SF_ERR_UNSUPPORTED, "list precedence moves: the list class must fit one wave's LDS slice with 16-bit elements");
        e = hipFuncSetAttribute((const void*)k_prec_evaluate_moves, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
        for (int64_t base = 0; base < n && e == hipSuccess; base += ctx->R) {
            const int chunk = (int)std::min<int64_t>(ctx->R, n - base);
            hipLaunchKernelGGL(k_prec_evaluate_moves, dim3(chunk), dim3(64), cv.total, ctx->stream, ctx->lm, ctx->pm, replica, d_moves, base, d_sc.p, d_do.p);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && ctx->xown_level >= 0) {  // the join of the two planning classes: its delta from the move's coordinates (k_cross_owner_evaluate_moves)
        hipLaunchKernelGGL(k_cross_owner_holders, dim3(1), dim3(256), 0, ctx->stream, ctx->lm, replica, ctx->sm.n, ctx->d_xown_tab);
        hipLaunchKernelGGL(k_cross_owner_evaluate_moves, dim3(grid), dim3(256), 0, ctx->stream, ctx->lm, ctx->sm.vals, ctx->sm.n, ctx->d_xown_tab, replica, d_moves, n,
                           ctx->xown_level, ctx->xown_weight, d_sc.p, d_do.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_sc.p, (size_t)n * ctx->levels * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_doable, d_do.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_rc(ctx, e);
}

// model gates of the compound-candidate surface (sf_step_evaluate_compound, sf_apply_compound, sf_step_decide*)
static int compound_model_gates(sf_ctx* ctx) {
    if (ctx->sm.grp_level >= 0 && ctx->sm.grp_mode >= 1)
        return fail(ctx, SF_ERR_UNSUPPORTED, "compound candidates on a load_balance / balance model (floating-point aggregate) are not chained on the device");
    if (ctx->sm.run_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "compound candidates on a consecutive-runs model are not chained on the device");
    return SF_OK;
}

// ScalarCandidateProvider surface: multi-edit candidates scored as ONE CompoundScalarMove each
int32_t sf_step_evaluate_compound(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, const int64_t* offsets, int64_t n,
                                  int64_t* out_scores, int32_t* out_doable) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_scalar_model) return fail(ctx, SF_ERR_INVALID, "compound scalar candidates need a scalar variable");
    if (replica < 0 || replica >= ctx->R || n < 0 || !offsets || !out_scores || !out_doable)
        return fail(ctx, SF_ERR_INVALID, "bad sf_step_evaluate_compound arguments");
    int rc;
    if ((rc = compound_model_gates(ctx))) return rc;
    if (n == 0) return SF_OK;
    if (offsets[0] != 0) return fail(ctx, SF_ERR_INVALID, "offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(ctx, SF_ERR_INVALID, "offsets must not decrease");
        if (offsets[i + 1] - offsets[i] > SF_COMPOUND_MAX) return fail(ctx, SF_ERR_UNSUPPORTED, "at most 8 edits per compound candidate on the device");
    }
    const int64_t total = offsets[n];
    if (total > 0 && !edits) return fail(ctx, SF_ERR_INVALID, "edits is NULL");
    for (int64_t k = 0; k < total; ++k)
        if (edits[k].kind != SF_MOVE_CHANGE) return fail(ctx, SF_ERR_INVALID, "a ScalarEdit is a SF_MOVE_CHANGE-shaped record");
    Scratch<sf_move_t> d_rec;
    Scratch<int64_t> d_off, d_sc;
    Scratch<int32_t> d_do;
    if ((rc = d_rec.upload(ctx, edits, (size_t)total)) || (rc = d_off.upload(ctx, offsets, (size_t)(n + 1))) || (rc = d_sc.alloc(ctx, (size_t)n * ctx->levels)) ||
        (rc = d_do.alloc(ctx, (size_t)n)))
        return rc;
    const int32_t* d_edits = (const int32_t*)d_rec.p;
    HIPCHK(ctx, launch_with_lds(k_scalar_evaluate_compound, dim3((int)((n + 255) / 256)), dim3(256), scalar_table_bytes(ctx), ctx->stream, ctx->sm, replica, d_edits,
                                d_off.p, n, d_sc.p, d_do.p));
    if (ctx->xown_level >= 0) {  // the join of the two planning classes: a scalar edit changes the A side's key
        hipLaunchKernelGGL(k_cross_owner_holders, dim3(1), dim3(256), 0, ctx->stream, ctx->lm, replica, ctx->sm.n, ctx->d_xown_tab);
        hipLaunchKernelGGL(k_cross_owner_evaluate_compound, dim3((int)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->sm.vals, ctx->sm.n, ctx->d_xown_tab, replica, d_edits,
                           d_off.p, n, ctx->levels, ctx->xown_level, ctx->xown_weight, d_sc.p, d_do.p);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_scores, d_sc.p, (size_t)n * ctx->levels * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_doable, d_do.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_rc(ctx, e);
}

// The join of the two planning classes under sf_apply / sf_apply_compound: its delta is priced on the state BEFORE the move (into ctx->d_xown_delta,
// SF_MAX_LEVELS words), and added to the committed score by xown_commit once the apply kernel has said the move went through (ctx->d_ok).
static int xown_price(sf_ctx* ctx, int32_t replica, const sf_move_t* records, int64_t n_records, const int64_t* compound_offsets) {
    if (ctx->xown_level < 0) return SF_OK;
    int rc;
    if (!ctx->d_xown_delta && (rc = dalloc(ctx, &ctx->d_xown_delta, (size_t)SF_MAX_LEVELS))) return rc;
    Scratch<sf_move_t> d_rec;
    Scratch<int64_t> d_off;
    if ((rc = d_rec.upload(ctx, records, (size_t)n_records))) return rc;
    if ((rc = hip_rc(ctx, hipMemsetAsync(ctx->d_xown_delta, 0, (size_t)SF_MAX_LEVELS * 8, ctx->stream)))) return rc;
    if (compound_offsets && (rc = d_off.upload(ctx, compound_offsets, 2))) return rc;
    hipLaunchKernelGGL(k_cross_owner_holders, dim3(1), dim3(256), 0, ctx->stream, ctx->lm, replica, ctx->sm.n, ctx->d_xown_tab);
    if (compound_offsets)  // ONE compound candidate: records [0, n_records)
        hipLaunchKernelGGL(k_cross_owner_evaluate_compound, dim3(1), dim3(256), 0, ctx->stream, ctx->sm.vals, ctx->sm.n, ctx->d_xown_tab, replica, (const int32_t*)d_rec.p,
                           d_off.p, (int64_t)1, ctx->levels, ctx->xown_level, ctx->xown_weight, ctx->d_xown_delta, (const int32_t*)nullptr);
    else
        hipLaunchKernelGGL(k_cross_owner_evaluate_moves, dim3(1), dim3(256), 0, ctx->stream, ctx->lm, ctx->sm.vals, ctx->sm.n, ctx->d_xown_tab, replica, (const int32_t*)d_rec.p,
                           (int64_t)1, ctx->xown_level, ctx->xown_weight, ctx->d_xown_delta, (const int32_t*)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the caller's host records may go away after this call)
    return hip_rc(ctx, e);
}
static void xown_commit(sf_ctx* ctx, int32_t replica) {
    if (ctx->xown_level < 0) return;
    hipLaunchKernelGGL(k_cross_owner_commit, dim3(1), dim3(1), 0, ctx->stream, ctx->lm.score + (size_t)replica * 4 + ctx->xown_level,
                       ctx->d_xown_delta + ctx->xown_level, ctx->d_ok);
}

int32_t sf_apply_compound(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, int64_t n_edits) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized || !edits || replica < 0 || replica >= ctx->R) return fail(ctx, SF_ERR_INVALID, "bad sf_apply_compound arguments");
    if (!ctx->has_scalar_model) return fail(ctx, SF_ERR_INVALID, "compound scalar candidates need a scalar variable");
    if (n_edits <= 0) return fail(ctx, SF_ERR_INVALID, "move is not doable");
    if (n_edits > SF_COMPOUND_MAX) return fail(ctx, SF_ERR_UNSUPPORTED, "at most 8 edits per compound candidate on the device");
    int rc;
    if ((rc = compound_model_gates(ctx))) return rc;
    for (int64_t k = 0; k < n_edits; ++k)
        if (edits[k].kind != SF_MOVE_CHANGE) return fail(ctx, SF_ERR_INVALID, "a ScalarEdit is a SF_MOVE_CHANGE-shaped record");
    if ((rc = alloc_search(ctx))) return rc;
    Scratch<sf_move_t> d_edits;
    if ((rc = d_edits.upload(ctx, edits, (size_t)n_edits))) return rc;
    const int64_t one_candidate[2] = {0, n_edits};
    if ((rc = xown_price(ctx, replica, edits, n_edits, one_candidate))) return rc;
    HIPCHK(ctx, launch_with_lds(k_scalar_apply_compound, dim3(1), dim3(64), scalar_table_bytes(ctx), ctx->stream, ctx->sm, replica, (const int32_t*)d_edits.p,
                                (int)n_edits, ctx->d_ok));
    xown_commit(ctx, replica);
    int32_t ok = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&ok, ctx->d_ok, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    if (!ok) return fail(ctx, SF_ERR_INVALID, "move is not doable");
    return SF_OK;
}

// One host-driven local-search step over a ScalarCandidateProvider's output (GroupedScalarMoveSelector; see the header).
static int32_t step_decide_impl(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, const int64_t* offsets, const int32_t* gates, int64_t n,
                                int32_t group_name_len, int64_t max_moves_per_step, int64_t* out_kept, int64_t* out_n_kept, int64_t* out_scores,
                                int32_t* out_flags, int64_t* out_consumed, int64_t* out_selected, bool cursor_order) {
    DeviceGuard _dev(ctx);
    if (ctx && ctx->xown_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide_gated: a model with the join of its two planning classes is searched by the fused engine only");
    if (!ctx || !ctx->initialized || replica < 0 || replica >= ctx->R || n < 0 || !offsets || !out_kept || !out_n_kept || !out_scores || !out_flags ||
        !out_consumed || !out_selected)
        return fail(ctx, SF_ERR_INVALID, "bad sf_step_decide arguments");
    if (!ctx->has_scalar_model || ctx->has_list_model) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide: scalar-only models (ScalarCandidate edits)");
    if (int rc = compound_model_gates(ctx)) return rc;
    if (ctx->vnd)
        return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide: not under variable neighborhood descent (the provider step runs an acceptor and a forager)");
    if (ctx->cfg.acceptor == SF_ACCEPT_TABU_SEARCH)
        return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide: not under TabuSearch (a compound candidate has no fixed-size move signature)");
    if (ctx->cfg.acceptor == SF_ACCEPT_SIMULATED_ANNEALING)
        return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide: HillClimbing, LateAcceptance, DiversifiedLateAcceptance, GreatDeluge or StepCountingHillClimbing");
    if (offsets[0] != 0) return fail(ctx, SF_ERR_INVALID, "offsets[0] must be 0");
    if (n >= ((int64_t)1 << 31)) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_step_decide: fewer than 2^31 candidates");
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(ctx, SF_ERR_INVALID, "offsets must not decrease");
    if (n > 0 && offsets[n] > 0 && !edits) return fail(ctx, SF_ERR_INVALID, "edits is NULL");
    for (int64_t k = 0; n > 0 && k < offsets[n]; ++k)
        if (edits[k].kind == SF_MOVE_SCALAR_RUIN) return fail(ctx, SF_ERR_UNSUPPORTED, SCALAR_RUIN_RECORD_REFUSAL);
    int rc = alloc_search(ctx);
    if (rc) return rc;
    SearchParams p = ctx->sp;
    fill_search_params(ctx, p);
    const ClassSpec& c = ctx->classes[ctx->scalar_desc];
    const int ne = ctx->sm.n;
    // the step's MoveStreamContext and the replica's working values (the cursor filters by is_doable_on)
    std::vector<int32_t> vals((size_t)ne);
    uint64_t step_index = 0, draws = 0;
    HIPCHK(ctx, hipMemcpyAsync(vals.data(), ctx->sm.vals + (size_t)replica * ne, (size_t)ne * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&step_index, p.step_index + replica, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&draws, p.seed_draws + replica, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t sseed = step_seed(p.random_seed + (uint64_t)replica, draws);
    if (ctx->d_explicit && (int64_t)draws < ctx->n_explicit) {
        HIPCHK(ctx, hipMemcpy(&sseed, ctx->d_explicit + (size_t)replica * ctx->n_explicit + draws, 8, hipMemcpyDeviceToHost));
    }
    const StreamCtx sctx{step_index, sseed, p.order};
    const int64_t cap = max_moves_per_step > 0 ? max_moves_per_step : 256;  // candidate-backed group (grouped_scalar.rs:27-40)
    // GroupedScalarCursor::activate, Candidates arm (grouped_scalar.rs:122-176)
    std::vector<int64_t> kept;
    auto legal = [&](int32_t e, int32_t to) {
        if (e < 0 || e >= ne) return false;
        if (to < 0) return to == -1 && c.allows_unassigned != 0;
        if (to >= c.n_values) return false;
        if (c.value_off.empty()) return true;
        for (uint32_t q = c.value_off[(size_t)e]; q < c.value_off[(size_t)e + 1]; ++q)
            if (c.value_list[q] == to) return true;
        return false;
    };
    for (int64_t o = 0; cursor_order && o < n; ++o) {  // a cursor's store: pull order, nothing skipped; malformed records are the caller's error
        const int64_t b = offsets[o], e = offsets[o + 1];
        if (e == b) return fail(ctx, SF_ERR_INVALID, "sf_step_decide_cursor: a candidate without edits (the cursor normalises its store)");
        if (e - b > SF_COMPOUND_MAX) return fail(ctx, SF_ERR_UNSUPPORTED, "at most 8 edits per compound candidate on the device");
        for (int64_t k = b; k < e; ++k) {
            if (edits[k].kind != SF_MOVE_CHANGE) return fail(ctx, SF_ERR_INVALID, "a ScalarEdit is a SF_MOVE_CHANGE-shaped record");
            for (int64_t j = b; j < k; ++j)
                if (edits[j].a == edits[k].a) return fail(ctx, SF_ERR_INVALID, "sf_step_decide_cursor: two edits on one entity (the cursor normalises its store)");
            if (!legal(edits[k].a, edits[k].value)) return fail(ctx, SF_ERR_INVALID, "sf_step_decide_cursor: an edit outside the entity's value range");
        }
        kept.push_back(o);
    }
    for (int64_t o = 0; !cursor_order && o < n && (int64_t)kept.size() < cap; ++o) {
        const int64_t idx = (int64_t)sctx.selection_index((uint32_t)o, (uint32_t)n, 0xC0A1E5CEAAA00001ULL ^ (uint64_t)group_name_len);  // apply_selection_order
        const int64_t b = offsets[idx], e = offsets[idx + 1];
        if (e == b) continue;
        if (e - b > SF_COMPOUND_MAX) return fail(ctx, SF_ERR_UNSUPPORTED, "at most 8 edits per compound candidate on the device");
        bool ok = true, changes = false;
        for (int64_t k = b; k < e && ok; ++k) {
            if (edits[k].kind != SF_MOVE_CHANGE) return fail(ctx, SF_ERR_INVALID, "a ScalarEdit is a SF_MOVE_CHANGE-shaped record");
            for (int64_t j = b; j < k; ++j) ok = ok && edits[j].a != edits[k].a;  // two edits on one (descriptor, entity, variable)
            ok = ok && legal(edits[k].a, edits[k].value);
            if (ok) changes = changes || vals[(size_t)edits[k].a] != edits[k].value;
        }
        if (!ok || !changes) continue;
        bool seen = false;
        for (int64_t q : kept) {
            if (offsets[q + 1] - offsets[q] != e - b) continue;
            bool same = true;
            for (int64_t k = 0; k < e - b && same; ++k) same = edits[offsets[q] + k].a == edits[b + k].a && edits[offsets[q] + k].value == edits[b + k].value;
            seen = seen || same;
        }
        if (seen) continue;
        kept.push_back(idx);
    }
    const int64_t nk = (int64_t)kept.size();
    *out_n_kept = nk;
    for (int64_t i = 0; i < nk; ++i) out_kept[i] = kept[(size_t)i];
    // kept candidates as their own CSR
    std::vector<sf_move_t> kedits;
    std::vector<int64_t> koff(1, 0);
    for (int64_t q : kept) {
        for (int64_t k = offsets[q]; k < offsets[q + 1]; ++k) kedits.push_back(edits[k]);
        koff.push_back((int64_t)kedits.size());
    }
    std::vector<int32_t> kgates;  // in pull order
    if (gates)
        for (int64_t q : kept) kgates.push_back(gates[q]);
    const size_t nk1 = (size_t)(nk > 0 ? nk : 1);
    Scratch<sf_move_t> d_rec;
    Scratch<int64_t> d_off, d_sc, d_res;
    Scratch<int32_t> d_do, d_fl, d_gates;  // d_gates stays NULL without gates
    if ((rc = d_rec.upload(ctx, kedits.data(), kedits.size())) || (rc = d_off.upload(ctx, koff.data(), (size_t)(nk + 1))) || (rc = d_sc.alloc(ctx, nk1 * ctx->levels)) ||
        (rc = d_do.alloc(ctx, nk1)) || (rc = d_fl.alloc(ctx, nk1)) || (rc = d_res.alloc(ctx, 2)))
        return rc;
    if ((rc = hip_rc(ctx, hipMemsetAsync(d_fl.p, 0, nk1 * 4, ctx->stream)))) return rc;
    if (!kgates.empty() && (rc = d_gates.upload(ctx, kgates.data(), kgates.size()))) return rc;
    const int32_t* d_edits = (const int32_t*)d_rec.p;
    if (nk > 0)
        HIPCHK(ctx, launch_with_lds(k_scalar_evaluate_compound, dim3((int)((nk + 255) / 256)), dim3(256), scalar_table_bytes(ctx), ctx->stream, ctx->sm, replica, d_edits,
                                    d_off.p, nk, d_sc.p, d_do.p));
    HIPCHK(ctx, launch_with_lds(k_scalar_step_decide, dim3(1), dim3(64), scalar_table_bytes(ctx), ctx->stream, ctx->sm, p, replica, d_edits, d_off.p, nk, d_sc.p, d_do.p,
                                d_fl.p, d_res.p, (const int32_t*)d_gates.p, ctx->hard_levels));
    hipError_t e = hipGetLastError();
    int64_t res[2] = {0, -1};
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res.p, 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && nk > 0) e = hipMemcpyAsync(out_scores, d_sc.p, (size_t)nk * ctx->levels * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && nk > 0) e = hipMemcpyAsync(out_flags, d_fl.p, (size_t)nk * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    *out_consumed = res[0];
    *out_selected = res[1];
    return SF_OK;
}

int32_t sf_step_decide(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, const int64_t* offsets, int64_t n, int32_t group_name_len,
                       int64_t max_moves_per_step, int64_t* out_kept, int64_t* out_n_kept, int64_t* out_scores, int32_t* out_flags,
                       int64_t* out_consumed, int64_t* out_selected) {
    return sf_step_decide_gated(ctx, replica, edits, offsets, nullptr, n, group_name_len, max_moves_per_step, out_kept, out_n_kept, out_scores, out_flags,
                                out_consumed, out_selected);
}
// the same step with Move::requires_hard_improvement / requires_score_improvement per candidate (gates[i]: bit 0 / bit 1)
int32_t sf_step_decide_gated(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, const int64_t* offsets, const int32_t* gates, int64_t n,
                             int32_t group_name_len, int64_t max_moves_per_step, int64_t* out_kept, int64_t* out_n_kept, int64_t* out_scores,
                             int32_t* out_flags, int64_t* out_consumed, int64_t* out_selected) {
    return step_decide_impl(ctx, replica, edits, offsets, gates, n, group_name_len, max_moves_per_step, out_kept, out_n_kept, out_scores, out_flags, out_consumed,
                            out_selected, false);
}
// the step over a cursor's own pull order (RuntimeProviderCursor, runtime/provider_cursor.rs:447-466): no activation is restated here --
// the cursor has rotated, normalised, deduplicated per provider scope and capped its store, and pushed doable moves only
// (provider_cursor.rs:420-437) -- so candidate i is pull i; see the header
int32_t sf_step_decide_cursor(sf_ctx* ctx, int32_t replica, const sf_move_t* edits, const int64_t* offsets, const int32_t* gates, int64_t n,
                              int64_t* out_scores, int32_t* out_flags, int64_t* out_consumed, int64_t* out_selected) {
    std::vector<int64_t> kept((size_t)(n > 0 ? n : 1));
    int64_t nk = 0;
    return step_decide_impl(ctx, replica, edits, offsets, gates, n, 0, 0, kept.data(), &nk, out_scores, out_flags, out_consumed, out_selected, true);
}

// sf_apply of one SF_MOVE_LIST_RUIN record: its launcher commits the ruin + recreate (one wavefront) and says whether the move was doable
static int apply_ruin(sf_ctx* ctx, int32_t replica, const sf_move_t* mv) {
    Scratch<sf_move_t> d_mv;
    Scratch<int64_t> d_sc;
    Scratch<int32_t> d_do;
    int rc;
    if ((rc = d_mv.upload(ctx, mv, 1)) || (rc = d_sc.alloc(ctx, 4)) || (rc = d_do.alloc(ctx, 1))) return rc;
    const std::vector<int32_t> which{0};
    if ((rc = ctx->pm.on ? launch_prec_ruin_moves(ctx, replica, (const int32_t*)d_mv.p, which, d_sc.p, d_do.p, 1)
                         : launch_ruin_moves(ctx, replica, (const int32_t*)d_mv.p, which, d_sc.p, d_do.p, 1)))
        return rc;
    int32_t ok = 0;
    if ((rc = hip_rc(ctx, hipMemcpy(&ok, d_do.p, 4, hipMemcpyDeviceToHost)))) return rc;
    if (!ok) return fail(ctx, SF_ERR_INVALID, "move is not doable");
    // the recreate by the precedence constraint: the committed scores are refreshed from the new lists
    return ctx->pm.on ? run_evaluate_all(ctx, nullptr, 1) : SF_OK;
}

int32_t sf_apply(sf_ctx* ctx, int32_t replica, const sf_move_t* mv) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized || !mv || replica < 0 || replica >= ctx->R)
        return fail(ctx, SF_ERR_INVALID, "bad sf_apply arguments");
    if (ctx->xown_level >= 0 && mv->kind == SF_MOVE_LIST_RUIN) return fail(ctx, SF_ERR_UNSUPPORTED, "the join of the two planning classes is not priced by a ruin's recreate");
    if (mv->kind == SF_MOVE_SCALAR_RUIN) return fail(ctx, SF_ERR_UNSUPPORTED, SCALAR_RUIN_RECORD_REFUSAL);
    int rc = alloc_search(ctx);
    if (rc) return rc;
    if (mv->kind == SF_MOVE_LIST_RUIN) {  // committed ruin + recreate: its own kernel
        if (!ctx->has_list_model) return fail(ctx, SF_ERR_INVALID, "list move on a model without a list variable");
        if (!ctx->pm.on && ctx->has_scalar_model) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_apply of a list ruin on a mixed model");
        return apply_ruin(ctx, replica, mv);
    }
    if (mv->kind == SF_MOVE_LIST_MULTI_SWAP) {  // the lists are pairwise different: the swaps commute, so they are committed one after the other
        if (!ctx->has_list_model) return fail(ctx, SF_ERR_INVALID, "list move on a model without a list variable");
        if (mv->a < 1 || mv->a > 3) return fail(ctx, SF_ERR_INVALID, "multi-swap: 1..3 swaps");
        sf_move_t one[3];
        const int32_t words[3] = {mv->a_pos, mv->b, mv->b_pos};
        for (int q = 0; q < mv->a; ++q) {
            const uint32_t w = (uint32_t)words[q];
            const int32_t dl = (int32_t)(int8_t)(((uint32_t)mv->value >> (8 * q)) & 0xFFu);
            one[q] = sf_move_t{SF_MOVE_LIST_SWAP, (int32_t)(w & 0xFFFFu), (int32_t)(w >> 16), (int32_t)(w & 0xFFFFu), (int32_t)(w >> 16) + dl, -1};
            for (int q2 = 0; q2 < q; ++q2)
                if (one[q2].a == one[q].a) return fail(ctx, SF_ERR_INVALID, "multi-swap: the swaps must touch pairwise different lists");
            if (dl == 0 || one[q].b_pos < 0) return fail(ctx, SF_ERR_INVALID, "multi-swap: a swap needs two different positions");
        }
        for (int q = 0; q < mv->a; ++q) {
            const int32_t rc2 = sf_apply(ctx, replica, &one[q]);
            if (rc2 != SF_OK) {
                for (int q2 = q - 1; q2 >= 0; --q2) (void)sf_apply(ctx, replica, &one[q2]);  // a swap is its own inverse
                return rc2;
            }
        }
        return SF_OK;
    }
    const bool list_move = (mv->kind >= SF_MOVE_LIST_CHANGE && mv->kind <= SF_MOVE_KOPT) || mv->kind == SF_MOVE_LIST_PERMUTE;
    if (list_move && !ctx->has_list_model) return fail(ctx, SF_ERR_INVALID, "list move on a model without a list variable");
    if (!list_move && !ctx->has_scalar_model) return fail(ctx, SF_ERR_INVALID, "scalar move on a model without a scalar variable");
    if (list_move) {
        if (mv->a < 0 || mv->a >= ctx->lm.V || mv->b < 0 || (mv->kind != SF_MOVE_KOPT && mv->b >= ctx->lm.V) || mv->a_pos < 0 ||
            mv->b_pos < 0)
            return fail(ctx, SF_ERR_INVALID, "move out of range");
        if (mv->kind == SF_MOVE_KOPT && (mv->value < 0 || mv->value >= 7))
            return fail(ctx, SF_ERR_INVALID, "3-opt move: value is the reconnection pattern 0..6");
        if (mv->kind == SF_MOVE_LIST_PERMUTE && (mv->a != mv->b || mv->b_pos - mv->a_pos < 2 || mv->b_pos - mv->a_pos > 8 || mv->value < 1))
            return fail(ctx, SF_ERR_INVALID, "list permute move: a window of 2..8 positions of one list and a permutation rank >= 1");
        if (mv->kind == SF_MOVE_SUBLIST_CHANGE && (mv->value <= mv->a_pos || mv->value - mv->a_pos > 255))
            return fail(ctx, SF_ERR_INVALID, "sublist move: value must be the segment end (segment of 1..255 elements)");
        if (mv->kind == SF_MOVE_SUBLIST_SWAP && (mv->value <= 0 || (mv->value & 0xFFFF) == 0 || (mv->value & 0xFFFF) > 255 ||
                                                 (mv->value >> 16) == 0 || (mv->value >> 16) > 255))
            return fail(ctx, SF_ERR_INVALID, "sublist swap: value packs the two segment sizes (1..255 each)");
        if ((rc = xown_price(ctx, replica, mv, 1, nullptr))) return rc;
        hipLaunchKernelGGL(k_list_apply, dim3(1), dim3(256), 0, ctx->stream, ctx->lm, replica, mv->kind,
                           (uint32_t)mv->a, (uint32_t)mv->a_pos, (uint32_t)mv->b, (uint32_t)mv->b_pos,
                           (uint32_t)(mv->value > 0 ? mv->value : 0), ctx->d_ok);
        if (ctx->pm.on)  // a move that was not doable left the lists alone: the refresh then changes nothing
            hipLaunchKernelGGL(k_prec_after_apply, dim3(1), dim3(64), 0, ctx->stream, ctx->lm, ctx->pm, replica);
    } else {
        if ((rc = xown_price(ctx, replica, mv, 1, nullptr))) return rc;
        HIPCHK(ctx, launch_with_lds(k_scalar_apply, dim3(1), dim3(64), scalar_table_bytes(ctx), ctx->stream, ctx->sm, replica, mv->kind, mv->a, mv->b, mv->value,
                                    ctx->d_ok));
    }
    xown_commit(ctx, replica);
    HIPCHK(ctx, hipGetLastError());
    int32_t ok = 0;
    HIPCHK(ctx, hipMemcpyAsync(&ok, ctx->d_ok, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (!ok) return fail(ctx, SF_ERR_INVALID, "move is not doable");
    return SF_OK;
}

}  // extern "C"
